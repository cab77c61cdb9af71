"""A stream programme as a ticket of the asynchronous ring
(mirsha_streams_submit, one lane per segment between Sum-then-Reset / Reset
ops): HashStreams.submit / submit_device / submit_flush and StreamLog's
submit_cycle.  Expected values come from hashlib hashers, one per stream
(tests/streamref.py), never from the code under test; a stream's state is
checked as its exported 108 bytes and by a later Sum.  Every case is a few
launches over a few KB."""
import ctypes
import hashlib

import numpy as np
import pytest

from mirbft_amd import (STREAM_RESET, STREAM_SUM, STREAM_SUM_RESET, STREAM_WRITE, Actions, Checkpoint, CheckpointChains,
                        Commit, CommitBatch, DeviceLog, HashRequest, HashStreams, MirshaError, Processor,
                        ProcessorWorkPool, StreamLog, StreamTicket, _lib, stream_seg_plan)
from mirbft_amd.hashdata import uint64_to_bytes
from streamref import Walker, marshal_of, run_ref

pytestmark = pytest.mark.gpu

EMPTY = hashlib.sha256(b"").digest()
W, S, SR, R = STREAM_WRITE, STREAM_SUM, STREAM_SUM_RESET, STREAM_RESET
FIRST, LAST = _lib.MIRSHA_STREAM_SEG_FIRST, _lib.MIRSHA_STREAM_SEG_LAST
CP = _lib.MIRSHA_COMMIT_CHECKPOINT


def values(rows):
    return [r.tobytes() for r in rows]


def preload(hs, ref, rng, fills):
    """Streams {s: fill} get `fill` bytes written (synchronously) first."""
    ops, parts, at = [], [], 0
    for s, n in fills.items():
        data = rng.bytes(n)
        ops.append((s, W, at, n))
        parts.append(data)
        at += n
        ref[s].run(W, data)
    if ops:
        hs.run(ops, b"".join(parts))


def check_states(hs, ref):
    """Every stream's exported state, then a Sum of each (which leaves it)."""
    n = len(ref)
    assert values(hs.export_state(np.arange(n))) == [marshal_of(r.written) for r in ref]
    assert values(hs.run([(s, S) for s in range(n)])) == [r.h.digest() for r in ref]


def interleave(rng, programmes):
    """[(stream, [(kind, off, len)...])] -> ops in a random interleaving that
    keeps every stream's own order."""
    owner = np.concatenate([np.full(len(p), k, dtype=np.int64) for k, (_, p) in enumerate(programmes)] or
                           [np.empty(0, dtype=np.int64)])
    rng.shuffle(owner)
    at = [0] * len(programmes)
    ops = []
    for k in owner:
        s, prog = programmes[k]
        ops.append((s,) + tuple(prog[at[k]]))
        at[k] += 1
    return ops


def random_ops(rng, n, n_ops, arena_len, p_cut=0.2):
    ops = []
    for _ in range(n_ops):
        s = int(rng.integers(0, n))
        x = rng.random()
        if x < p_cut / 2:
            ops.append((s, SR, 0, 0))
        elif x < p_cut:
            ops.append((s, R, 0, 0))
        elif x < p_cut + 0.1:
            ops.append((s, S, 0, 0))
        else:
            ln = int(rng.integers(0, min(arena_len, 150) + 1))
            ops.append((s, W, int(rng.integers(0, arena_len - ln + 1)), ln))
    return ops


def device_arena(arena, lead=0):
    """The arena in device memory at an address = lead (mod 256); (tensor, address)."""
    import torch

    t = torch.frombuffer(bytearray(bytes(lead) + bytes(arena)), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    assert t.data_ptr() % 256 == 0
    return t, t.data_ptr() + lead


# ---- 1. segment classes -----------------------------------------------------------------

A = 1203  # the arena's size: not a multiple of 4
LENGTHS = (0, 1, 55, 56, 63, 64, 65, 119, 120, 128)  # one- and two-block padding


def segment_classes():
    """[(stored fill, [(kind, off, len)...])], one stream each.  Offsets are
    arena offsets: the device form reads the arena where it lies, so they are
    the alignments the kernel sees."""
    c = []
    # FIRST only, then LAST only; the FIRST segment arrives at a stored fill b > 0 with a
    # write range at arena offset 0: its window begins before the arena
    for b, n in ((5, 70), (63, 1), (17, 200)):
        c.append((b, [(W, 0, n), (SR, 0, 0), (W, 9, 30), (S, 0, 0)]))
    # FIRST | LAST, with and without a stored fill
    c.append((0, [(W, 3, 90), (S, 0, 0)]))
    c.append((40, [(W, 3, 90), (SR, 0, 0)]))
    # a non-FIRST segment whose first write lies at each arena alignment
    for a in range(4):
        c.append((11 + a, [(SR, 0, 0), (W, 100 + a, 37 + a), (S, 0, 0)]))
        c.append((0, [(W, 1, 2), (R, 0, 0), (W, 300 + a, 64), (SR, 0, 0), (W, 400 + a, 5)]))
    # a non-FIRST segment whose write ends at the arena's last byte
    c.append((7, [(R, 0, 0), (W, A - 45, 45), (SR, 0, 0), (W, A - 1, 1), (S, 0, 0)]))
    c.append((0, [(SR, 0, 0), (W, A - 130, 130), (S, 0, 0)]))
    # a non-FIRST (and non-LAST: neither) segment of each total length; 0 is SUM_RESET directly
    # after SUM_RESET, whose value is sha256(b"")
    for k, n in enumerate(LENGTHS):
        c.append((k % 3 * 20, [(W, 50, 10), (SR, 0, 0), (W, 500 + k, n), (SR, 0, 0), (W, 2, 3)]))
        c.append((0, [(SR, 0, 0), (W, 600 + k, n // 2), (W, 700, n - n // 2), (SR, 0, 0), (S, 0, 0)]))  # in two writes
    # a SUM in mid-segment, followed by more writes
    c.append((33, [(W, 0, 10), (SR, 0, 0), (W, 800, 60), (S, 0, 0), (W, 860, 70), (S, 0, 0), (W, 930, 1), (SR, 0, 0),
                   (W, 5, 5), (S, 0, 0), (W, 10, 5)]))
    # segments that end in RESET: in the middle, and as the stream's final entry (LAST stores Hasher())
    c.append((9, [(W, 0, 100), (R, 0, 0), (W, 100, 77), (S, 0, 0), (R, 0, 0)]))
    c.append((0, [(R, 0, 0), (R, 0, 0), (W, 64, 64), (R, 0, 0)]))
    return c


@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("together", [True, False], ids=["one_ticket", "one_ticket_per_class"])
def test_segment_classes(engine, together, form):
    rng = np.random.default_rng(91)
    classes = segment_classes()
    n = len(classes)
    arena = rng.bytes(A)
    hs = HashStreams(engine, n)
    ref = [Walker() for _ in range(n)]
    preload(hs, ref, rng, {s: b for s, (b, _) in enumerate(classes) if b})
    programmes = [(s, prog) for s, (_, prog) in enumerate(classes)]
    kinds = set()
    for s, prog in programmes:  # every kind of segment is there
        kinds |= set(int(f) for f in stream_seg_plan([(s,) + op for op in prog], n, A)[2])
    assert kinds == {0, FIRST, LAST, FIRST | LAST}
    calls = [interleave(rng, programmes)] if together else [interleave(rng, [p]) for p in programmes]
    if form == "device":
        keep, d_arena = device_arena(arena)
        submit = lambda ops: hs.submit_device(ops, d_arena, A, keep=keep)
    else:
        submit = lambda ops: hs.submit(ops, arena)
    tickets = [submit(ops) for ops in calls]  # all queued before any wait
    assert all(isinstance(t, StreamTicket) for t in tickets)
    got, want = [], []
    for t, ops in zip(tickets, calls):
        v = engine.wait(t)
        assert v is t.values and v.shape == (sum(1 for op in ops if op[1] in (S, SR)), 32)
        got += values(v)
        want += run_ref(ref, arena, ops)
    assert got == want and EMPTY in want
    check_states(hs, ref)
    hs.close()


@pytest.mark.parametrize("lead", [0, 1, 2, 3])
def test_device_arena_at_every_address_alignment(engine, lead):
    """The arena itself at an address = lead (mod 4): `shift` moves every window."""
    rng = np.random.default_rng(92 + lead)
    arena = rng.bytes(A)
    hs = HashStreams(engine, 6)
    ref = [Walker() for _ in range(6)]
    preload(hs, ref, rng, {0: 5, 1: 62, 4: 1})
    ops = [(0, W, 0, 90), (0, SR), (0, W, 0, 65), (0, S),               # offset 0 at a fill, and from Hasher()
           (1, R), (1, W, A - 67, 67), (1, S),                           # ends at the arena's last byte
           (2, SR), (2, W, 1, 55), (2, SR), (2, W, 2, 56), (2, SR), (2, W, 3, 64), (2, S),
           (4, W, A - 1, 1), (4, S)]
    keep, d_arena = device_arena(arena, lead)
    got = values(engine.wait(hs.submit_device(ops, d_arena, A, keep=keep)))
    assert got == run_ref(ref, arena, ops)
    check_states(hs, ref)
    hs.close()


# ---- 2. widths --------------------------------------------------------------------------

@pytest.mark.parametrize("total", [1, 63, 64, 65, 129])
def test_widths_one_segment_streams(engine, total):
    rng = np.random.default_rng(600 + total)
    arena = rng.bytes(700)
    hs = HashStreams(engine, total + 1)
    ref = [Walker() for _ in range(total + 1)]
    preload(hs, ref, rng, {s: 1 + s % 70 for s in range(0, total + 1, 2)})  # the last stream is named by no op
    programmes = []
    for s in range(total):
        prog = [(W, int(rng.integers(0, 500)), int(rng.integers(1, 200))) for _ in range(1 + s % 3)]
        prog.append([(S, 0, 0), (SR, 0, 0), (R, 0, 0)][s % 3])  # ends in a reset: still one segment
        programmes.append((s, prog))
    ops = interleave(rng, programmes)
    plan = stream_seg_plan(ops, total + 1, 700)
    assert plan[0].size == total and all(int(f) == FIRST | LAST for f in plan[2])
    assert values(engine.wait(hs.submit(ops, arena))) == run_ref(ref, arena, ops)
    check_states(hs, ref)
    hs.close()


@pytest.mark.parametrize("total", [63, 64, 65, 129, 257])
@pytest.mark.parametrize("fill", [12, 37], ids=["even_fill", "odd_fill"])
def test_widths_one_stream_over_several_waves(engine, total, fill):
    """Stream 2 of 5 with total - 1 resets and a trailing write: its first
    segment reads the stored row and its last one stores, waves apart.  Its
    four neighbours hold states of their own: 0 and 4 run one segment each in
    the same ticket, 1 and 3 are named by no op."""
    rng = np.random.default_rng(700 + total + fill)
    arena = rng.bytes(900)
    hs = HashStreams(engine, 5)
    ref = [Walker() for _ in range(5)]
    preload(hs, ref, rng, {0: 70, 1: fill + 1, 2: fill, 3: 64, 4: 3})
    prog = []
    for k in range(total - 1):  # the first segment sums what the stored fill began
        prog += [(W, int(rng.integers(0, 800)), int(rng.integers(1, 100))) for _ in range(k % 3 if k else 1)]
        prog.append((R, 0, 0) if k % 4 == 1 else (SR, 0, 0))
    prog.append((W, 11, 75))
    programmes = [(2, prog), (0, [(W, 0, 30), (S, 0, 0)]), (4, [(W, 30, 100), (S, 0, 0), (W, 1, 1)])]
    ops = interleave(rng, programmes)
    seg_stream, _, flags, *_ = stream_seg_plan(ops, 5, 900)
    assert seg_stream.size == total + 2 and flags[1] == FIRST and flags[total] == LAST
    # FIRST in lane 1, LAST in lane `total`: in different waves from 64 on
    assert values(engine.wait(hs.submit(ops, arena))) == run_ref(ref, arena, ops)
    check_states(hs, ref)
    hs.close()


# ---- 3. equivalence with the synchronous call, and both forms on one object ---------------

def test_equivalence_with_run_on_a_second_object(engine):
    rng = np.random.default_rng(93)
    n = 70
    a, b = HashStreams(engine, n), HashStreams(engine, n)
    ref = [Walker() for _ in range(n)]
    for cycle in range(4):
        arena = rng.bytes(int(rng.integers(1, 3000)))
        ops = random_ops(rng, n, int(rng.integers(0, 1200)), len(arena))
        want = run_ref(ref, arena, ops)
        assert values(a.run(ops, arena)) == want, cycle
        assert values(engine.wait(b.submit(ops, arena))) == want, cycle
        states = [marshal_of(r.written) for r in ref]
        assert values(a.export_state(np.arange(n))) == states and values(b.export_state(np.arange(n))) == states, cycle
    assert a.runs == b.runs == 4 and a.bytes_sent == b.bytes_sent > 0
    a.close()
    b.close()


def test_both_forms_on_one_object_in_turn(engine):
    """run, submit, run, export_state: the library orders each behind the
    ticket in flight, the caller never waits in between."""
    rng = np.random.default_rng(94)
    n = 9
    hs = HashStreams(engine, n)
    ref = [Walker() for _ in range(n)]
    pending = []
    for step in range(6):
        arena = rng.bytes(2000)
        ops = random_ops(rng, n, 150, 2000)
        assert values(hs.run(ops, arena)) == run_ref(ref, arena, ops), step
        ops = random_ops(rng, n, 300, 2000, p_cut=0.4)
        pending.append((hs.submit(ops, arena), run_ref(ref, arena, ops)))
        ops = random_ops(rng, n, 80, 2000)
        assert values(hs.run(ops, arena)) == run_ref(ref, arena, ops), step
        assert values(hs.export_state(np.arange(n))) == [marshal_of(r.written) for r in ref], step
        if step == 3:  # import behind a ticket too
            hs.submit([(0, W, 0, 77)], arena)
            ref[0].run(W, arena[:77])
            hs.import_state([0], np.frombuffer(marshal_of(b"xyz"), dtype=np.uint8))
            ref[0] = Walker(b"xyz")
    for t, want in pending:  # values of tickets retired long ago are still theirs
        assert values(engine.wait(t)) == want
    check_states(hs, ref)
    hs.close()


# ---- 4. where the values land -----------------------------------------------------------

@pytest.mark.parametrize("where", ["pinned_aligned", "pinned_offset_8", "pageable"])
def test_values_out_memory_kinds(engine, where):
    rng = np.random.default_rng(95)
    n = 6
    hs = HashStreams(engine, n)
    ref = [Walker() for _ in range(n)]
    arena = rng.bytes(1500)
    ops = random_ops(rng, n, 300, 1500, p_cut=0.3)
    k = sum(1 for op in ops if op[1] in (S, SR))
    assert k > 10
    if where == "pageable":
        out = np.zeros((k, 32), dtype=np.uint8)
    else:
        raw = engine.host_empty(32 * k + 16)
        assert raw.ctypes.data % 16 == 0
        at = 8 if where == "pinned_offset_8" else 0
        out = raw[at:at + 32 * k].reshape(k, 32)
        out[:] = 0
    t = hs.submit(ops, arena, out=out)
    assert t.values is out
    assert values(engine.wait(t)) == run_ref(ref, arena, ops)
    check_states(hs, ref)
    with pytest.raises(ValueError):
        hs.submit(ops, arena, out=np.zeros((k + 1, 32), dtype=np.uint8))
    hs.close()


# ---- 5. the device form behind the hashing ------------------------------------------------

def test_submit_device_over_digests_hashed_just_before(engine):
    """Request digests written by hash_batch_device are streamed where they
    lie, with no synchronisation between the two calls."""
    import torch

    rng = np.random.default_rng(96)
    n_req, n = 64, 5
    ln = rng.integers(0, 300, n_req).astype(np.uint32)
    off = np.zeros(n_req, dtype=np.uint64)
    np.cumsum(ln[:-1].astype(np.uint64), out=off[1:])
    arena = rng.integers(0, 256, int(ln.sum()) + 1, dtype=np.uint8)
    host = b"".join(hashlib.sha256(arena[int(o):int(o) + int(k)].tobytes()).digest() for o, k in zip(off, ln))
    d_arena = torch.from_numpy(arena).cuda()
    d_off = torch.from_numpy(off.view(np.int64)).cuda()
    d_len = torch.from_numpy(ln.view(np.int32)).cuda()
    d_out = torch.zeros((n_req, 32), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ops = []  # whole digests, half digests and runs of digests, checkpoints in between
    for _ in range(400):
        s, x = int(rng.integers(0, n)), rng.random()
        if x < 0.15:
            ops.append((s, SR, 0, 0))
        else:
            d = int(rng.integers(0, n_req))
            ops.append((s, W, 32 * d + (16 if x < 0.3 else 0), 16 if x < 0.45 else min(96, 32 * (n_req - d))))
    hs = HashStreams(engine, n)
    ref = [Walker() for _ in range(n)]
    engine.hash_batch_device(d_arena.data_ptr(), arena.size, d_off.data_ptr(), d_len.data_ptr(), None, n_req,
                             d_out.data_ptr())
    t = hs.submit_device(ops, d_out.data_ptr(), 32 * n_req, keep=d_out)  # behind the hashing, no sync
    want = run_ref(ref, host, ops)
    assert values(engine.wait(t)) == want and len(want) > 10
    check_states(hs, ref)
    assert hs.bytes_sent == 0  # nothing crossed PCIe but the ops
    hs.close()


# ---- 6. the ring ------------------------------------------------------------------------

def test_ring_six_tickets_then_the_last_and_reverse_waits(engine):
    rng = np.random.default_rng(97)
    n = 7
    hs = HashStreams(engine, n)
    ref = [Walker() for _ in range(n)]
    for order in ("last_only", "reverse"):
        tickets, want = [], []
        for _ in range(6):  # more than the four slots: the fifth and sixth retire the oldest
            arena = rng.bytes(1000)
            ops = random_ops(rng, n, 200, 1000)
            tickets.append(hs.submit(ops, arena))
            want.append(run_ref(ref, arena, ops))
        assert [t.value for t in tickets] == list(range(tickets[0].value, tickets[0].value + 6))
        if order == "last_only":
            engine.wait(tickets[-1])  # retires every earlier ticket, in order
        else:
            for t in reversed(tickets):
                engine.wait(t)
        assert [values(t.values) for t in tickets] == want
        assert all(engine.poll(t) for t in tickets)  # retired
    fresh = hs.submit([(0, W, 0, 3), (0, SR)], b"abc")
    want = run_ref(ref, b"abc", [(0, W, 0, 3), (0, SR)])
    assert isinstance(engine.poll(fresh), bool)  # either answer is right for a fresh ticket
    assert values(engine.wait(fresh)) == want and engine.poll(fresh)
    # programmes without an active stream: valid tickets, nothing launched, states unchanged
    t1 = hs.submit([(0, W, 0, 0), (3, W, 2, 0)], b"abc")
    t2 = hs.submit([])
    assert t2.value == t1.value + 1 == fresh.value + 2
    assert engine.wait(t2).shape == (0, 32) and engine.wait(t1).shape == (0, 32)
    check_states(hs, ref)
    hs.close()


def test_ring_stream_tickets_between_hashing_and_commit_tickets(engine):
    rng = np.random.default_rng(98)
    n = 5
    hs, ch = HashStreams(engine, n), CheckpointChains(engine, n)
    ref = [Walker() for _ in range(n)]
    cref = [hashlib.sha256() for _ in range(n)]
    sha = lambda parts: hashlib.sha256(b"".join(parts)).digest()

    def commit_ref(table, oc, od):
        out = []
        for c, d in zip(oc.tolist(), od.tolist()):
            if d == CP:
                out.append(cref[c].digest())
                cref[c] = hashlib.sha256()
            else:
                cref[c].update(table[d].tobytes())
        return out

    issued = []  # (kind, ticket, expected)
    for round_ in range(3):
        reqs = [[rng.bytes(int(k)) for k in rng.integers(0, 120, 2)] for _ in range(70)]
        issued.append(("slices", engine.submit_slices(reqs), [sha(r) for r in reqs]))
        arena = rng.bytes(1500)
        ops = random_ops(rng, n, 300, 1500)
        issued.append(("stream", hs.submit(ops, arena), run_ref(ref, arena, ops)))
        table = rng.integers(0, 256, (48, 32), dtype=np.uint8)
        oc = rng.integers(0, n, 200).astype(np.uint32)
        od = rng.integers(0, 48, 200).astype(np.uint32)
        od[rng.random(200) > 0.9] = CP
        issued.append(("commit", ch.submit_commit(table, oc, od), commit_ref(table, oc, od)))
        ops = random_ops(rng, n, 50, 1500, p_cut=0.5)
        issued.append(("stream", hs.submit(ops, arena), run_ref(ref, arena, ops)))
        ln = rng.integers(0, 200, 90).astype(np.uint32)
        off = np.zeros(90, dtype=np.uint64)
        np.cumsum(ln[:-1].astype(np.uint64), out=off[1:])
        bytes_ = rng.integers(0, 256, int(ln.sum()) + 1, dtype=np.uint8)
        issued.append(("batch", engine.submit_batch(bytes_, off, ln),
                       [hashlib.sha256(bytes_[int(o):int(o) + int(k)].tobytes()).digest() for o, k in zip(off, ln)]))
    assert [t.value for _, t, _ in issued] == list(range(issued[0][1].value, issued[0][1].value + len(issued)))
    for kind, t, want in reversed(issued):
        assert values(engine.wait(t)) == want, kind
    check_states(hs, ref)
    assert values(ch.sum(np.arange(n, dtype=np.uint32))) == [r.digest() for r in cref]
    hs.close()
    ch.close()


# ---- 7. validation failures -------------------------------------------------------------

def test_validation_failures_queue_nothing(engine):
    rng = np.random.default_rng(99)
    data = rng.bytes(128)
    hs = HashStreams(engine, 4)
    ref = [Walker() for _ in range(4)]
    hs.run([(s, W, s, 40 + s) for s in range(4)], data)
    for s in range(4):
        ref[s].run(W, data[s:s + 40 + s])
    t0 = hs.submit([])  # an empty programme: a ticket all the same
    good = [(0, W, 0, 64), (1, SR), (2, R)]
    for bad, word in (((4, W, 0, 1), r"op_stream\[3\] = 4 >= 4"), ((0, 4, 0, 0), r"op_kind\[3\] = 4 is no kind"),
                      ((3, W, 100, 29), "op 3 writes"), ((3, W, 129, 0), "op 3 writes")):
        with pytest.raises(MirshaError, match=word) as e:
            hs.submit(good + [bad] + good, data)
        assert e.value.code == _lib.MIRSHA_EINVAL
    # sums without values_out: the raw call (the Python layer always passes one)
    os_ = np.asarray([0, 1, 2], dtype=np.uint32)
    ok = np.asarray([W, SR, W], dtype=np.uint32)
    oo = np.asarray([0, 0, 5], dtype=np.uint64)
    ol = np.asarray([9, 0, 7], dtype=np.uint32)
    k, t = ctypes.c_uint32(77), ctypes.c_uint64(77)
    arena = np.frombuffer(data, dtype=np.uint8)
    with pytest.raises(MirshaError, match="NULL values_out"):
        engine._check(engine._lib.mirsha_streams_submit(engine.ctx, hs.handle, arena.ctypes.data, arena.size,
                                                        os_.ctypes.data, ok.ctypes.data, oo.ctypes.data,
                                                        ol.ctypes.data, 3, None, ctypes.byref(k), ctypes.byref(t)))
    assert t.value == 77  # no ticket was handed out
    other = HashStreams(engine, 1)
    with pytest.raises(MirshaError):
        other.submit([(1, S)])
    other.close()
    ops = list(zip(os_.tolist(), ok.tolist(), oo.tolist(), ol.tolist()))
    t1 = hs.submit(ops, data)
    assert t1.value == t0.value + 1  # the failures consumed no ticket
    assert values(engine.wait(t1)) == run_ref(ref, data, ops)
    assert engine.poll(t0)
    check_states(hs, ref)  # ... and left every state as it was
    hs.close()


# ---- 8. hashers -------------------------------------------------------------------------

def test_submit_flush_of_a_hundred_hashers_over_three_steps(engine):
    rng = np.random.default_rng(100)
    hs = HashStreams(engine, 100)
    hashers = [hs.hasher() for _ in range(100)]
    refs = [hashlib.sha256() for _ in range(100)]
    tickets, want = [], []
    for step in range(3):
        for k, (h, r) in enumerate(zip(hashers, refs)):
            if step == 1 and k % 7 == 0:
                h.reset()
                refs[k] = r = hashlib.sha256()
            for _ in range(int(rng.integers(0, 3))):
                chunk = rng.bytes(int(rng.integers(0, 150)))
                h.write(chunk)
                r.update(chunk)
        order = [int(i) for i in rng.permutation(100)]
        tickets.append(hs.submit_flush([hashers[i] for i in order]))  # no wait between the steps
        want.append([refs[i].digest() for i in order])
        assert all(not h._pending and not h._reset for h in hashers)  # sent
    assert hs.runs == 3
    for t, w in zip(reversed(tickets), reversed(want)):
        assert isinstance(t, StreamTicket) and values(engine.wait(t)) == w
    # a refused submission leaves the hashers pending
    hashers[3].write(b"abc")
    hashers[5].reset()
    stream, hashers[4].stream = hashers[4].stream, 100  # no such stream
    with pytest.raises(MirshaError):
        hs.submit_flush(hashers[3:6])
    assert hashers[3]._pending == [b"abc"] and hashers[5]._reset
    hashers[4].stream = stream
    refs[3].update(b"abc")
    got = values(engine.wait(hs.submit_flush(hashers[3:6])))
    assert got == [refs[3].digest(), refs[4].digest(), EMPTY]
    assert engine.wait(hs.submit_flush(hashers[:2], sums=False)).shape == (0, 32)
    hs.close()


# ---- 9. Processor / ProcessorWorkPool with a StreamLog ------------------------------------

def sha(parts):
    return hashlib.sha256(b"".join(parts)).digest()


def seq_and_digests(batch):
    """An application-defined Apply: the sequence number, then the non-null digests."""
    return [uint64_to_bytes(batch.seq_no)] + [d for d in batch.digests if d]


class AppState:
    """What the log's streams hold, restated on hashlib."""

    def __init__(self, entry_data=None):
        self.active = hashlib.sha256()
        self.entry_data = entry_data or (lambda batch: [d for d in batch.digests if d])

    def commit(self, commits):
        out = []
        for c in commits:
            if c.batch is not None:
                self.active.update(b"".join(self.entry_data(c.batch)))
            else:
                out.append(self.active.digest())
                self.active = hashlib.sha256()
        return out


def six_cycles(seed):
    """Hashes, a cycle without commits, a cycle with only commits, checkpoints
    in the middle of a cycle's list."""
    rng = np.random.default_rng(seed)
    cycles, seq = [], 0
    for cycle in range(6):
        reqs = [HashRequest(data=[rng.bytes(int(k)) for k in rng.integers(0, 90, 3)], origin=(cycle, i))
                for i in range(0 if cycle == 4 else 25)]
        commits = []
        for _ in range(0 if cycle == 2 else 7):
            seq += 1
            digests = [None if rng.random() < 0.15 else rng.bytes(32) for _ in range(int(rng.integers(0, 6)))]
            commits.append(Commit(batch=CommitBatch(digests, seq_no=seq)))
            if seq % 3 == 0:
                commits.append(Commit(checkpoint=Checkpoint(seq_no=seq)))
        cycles.append((reqs, commits))
    return cycles


def check_cycle(res, reqs, commits, want_values):
    assert [r.digest for r in res.digests] == [sha(q.data) for q in reqs]
    asked = [c for c in commits if c.checkpoint is not None]
    assert [r.value for r in res.checkpoints] == want_values
    assert [r.commit for r in res.checkpoints] == asked


class SpyLog(StreamLog):
    """Counts which of the log's two forms the Processor calls."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.calls = {"commit_cycle": 0, "submit_cycle": 0}

    def commit_cycle(self, commits):
        self.calls["commit_cycle"] += 1
        return super().commit_cycle(commits)

    def submit_cycle(self, commits):
        self.calls["submit_cycle"] += 1
        return super().submit_cycle(commits)


@pytest.mark.parametrize("cls", [Processor, ProcessorWorkPool])
@pytest.mark.parametrize("entry_data", [None, seq_and_digests], ids=["digests", "application_defined"])
def test_processor_with_a_stream_log_async_commits_on_and_off(engine, cls, entry_data):
    cycles = six_cycles(101)
    state = AppState(entry_data)
    want = [state.commit(c) for _, c in cycles]
    assert sum(map(len, want)) >= 8
    with_commits = sum(1 for _, c in cycles if c)
    results = {}
    for flag in (False, True):
        log = SpyLog(engine, n_nodes=3, node=1, entry_data=entry_data)
        p = cls(engine=engine, log=log, async_commits=flag)
        pend = [p.submit(Actions(hash=r, commits=c)) for r, c in cycles]
        got = [None] * len(cycles)
        for k in reversed(range(len(cycles))):  # cycles committed in submission order all the same
            got[k] = pend[k].wait()
        for res, (reqs, commits), w in zip(got, cycles, want):
            check_cycle(res, reqs, commits, w)
        # with the flag on, submit_cycle is the call made
        assert log.calls == ({"commit_cycle": 0, "submit_cycle": with_commits} if flag else
                             {"commit_cycle": with_commits, "submit_cycle": 0})
        assert values(log.streams.run([(s, S) for s in range(3)])) == [state.active.digest()] * 3
        results[flag] = [([r.digest for r in res.digests], [r.value for r in res.checkpoints]) for res in got]
        log.close()
    assert results[True] == results[False]


def test_work_pool_process_with_a_stream_log_equals_device_log(engine):
    cycles = six_cycles(102)
    a, b = SpyLog(engine, n_nodes=4, node=2), DeviceLog(engine, n_nodes=4, node=2)
    pa = ProcessorWorkPool(engine=engine, log=a, async_commits=True)
    pb = ProcessorWorkPool(engine=engine, log=b, async_commits=True)
    state = AppState()
    ran = []
    for reqs, commits in cycles:
        ra = pa.process(Actions(hash=reqs, commits=commits), overlap=lambda: ran.append(1))
        rb = pb.process(Actions(hash=reqs, commits=commits))
        check_cycle(ra, reqs, commits, state.commit(commits))
        assert [r.value for r in ra.checkpoints] == [r.value for r in rb.checkpoints]
        if commits:
            assert np.array_equal(a.values, b.values) and a.values.shape[1:] == (4, 32)
    assert len(ran) == 6 and a.calls["commit_cycle"] == 0 and a.calls["submit_cycle"] == 5
    # the four nodes' writes name the same ranges: a cycle's bytes are sent once
    assert a.streams.bytes_sent == sum(len(d) for _, cs in cycles for c in cs if c.batch for d in c.batch.digests if d)
    a.close()
    b.close()
