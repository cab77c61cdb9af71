"""A stream programme under SHA-512/256 as a ticket of the asynchronous ring
(mirsha_streams_submit / _submit_device on streams of
mirsha_streams_create_hasher; sha512_streams_seg_kernel, one lane per segment
between Sum-then-Reset / Reset ops).  Expected values come from hashlib
hashers, one per stream (tests/stream512ref.py), never from the code under
test; a stream's state is checked as its exported 204 bytes and by a later Sum.
Every case is a few launches over a few KB."""
import hashlib

import numpy as np
import pytest

from mirbft_amd import (STREAM_RESET, STREAM_SUM, STREAM_SUM_RESET, STREAM_WRITE, Engine, HashStreams, _lib,
                        stream_seg_plan)
from stream512ref import NAME, Walker, marshal_of, run_ref

pytestmark = pytest.mark.gpu

W, S, SR, R = STREAM_WRITE, STREAM_SUM, STREAM_SUM_RESET, STREAM_RESET
FIRST, LAST = _lib.MIRSHA_STREAM_SEG_FIRST, _lib.MIRSHA_STREAM_SEG_LAST


def H(b) -> bytes:
    return hashlib.new(NAME, bytes(b)).digest()


@pytest.fixture(scope="module")
def own(engine):
    """An engine of this module's own (after the session's, so torch's runtime
    came up first): a failing test cannot leave the shared one on SHA-512/256."""
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture()
def eng(own):
    own.set_hasher(NAME)
    yield own
    own.set_hasher("sha256")


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
            ln = int(rng.integers(0, min(arena_len, 300) + 1))
            ops.append((s, W, int(rng.integers(0, arena_len - ln + 1)), ln))
    return ops


def device_arena(arena, lead=0):
    import torch

    t = torch.frombuffer(bytearray(bytes(lead) + bytes(arena)), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    return t, t.data_ptr() + lead


# ---- submit equals run: 0, 1 and 4 Sum-then-Resets per stream ------------------------------

@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("resets", [0, 1, 4])
def test_submit_equals_run(eng, resets, form):
    """Stream s arrives at fill s (every fill of the block and a few beyond),
    then runs `resets` + 1 stretches of writes around the block's edges."""
    rng = np.random.default_rng(900 + resets)
    n, A = 140, 1203  # A: not a multiple of 4
    arena = rng.bytes(A)
    a, b = HashStreams(eng, n), HashStreams(eng, n)
    ref = [Walker() for _ in range(n)]
    fills = {s: s for s in range(1, n)}
    preload(a, ref, rng, fills)
    b.import_state(np.arange(n), a.export_state(np.arange(n)))
    lens = (0, 1, 111, 112, 113, 127, 128, 129, 255, 257)
    ops = []
    for k in range(resets + 1):
        for s in range(n):
            ln = lens[(s + k) % len(lens)]
            ops.append((s, W, int(rng.integers(0, A - ln + 1)) if (s + k) % 7 else A - ln, ln))
            if s % 3 == 0:
                ops.append((s, S, 0, 0))
        if k < resets:
            ops += [(s, SR, 0, 0) for s in range(n)]
    ops += [(s, S, 0, 0) for s in range(n)]
    want = run_ref(ref, arena, ops)
    assert values(a.run(ops, arena)) == want
    if form == "device":
        t, at = device_arena(arena, 1 + resets % 3)
        got = eng.wait(b.submit_device(ops, at, A, keep=t))
    else:
        got = eng.wait(b.submit(ops, arena))
    assert values(got) == want
    states = [marshal_of(r.written) for r in ref]
    assert values(a.export_state(np.arange(n))) == states and values(b.export_state(np.arange(n))) == states
    a.close()
    b.close()


# ---- a stream's FIRST and LAST segment in different waves: the snapshot copy ----------------

@pytest.mark.parametrize("total", [64, 65, 129])
@pytest.mark.parametrize("fill", [12, 127], ids=["even_fill", "odd_fill"])
def test_one_stream_over_several_waves(eng, total, fill):
    """Stream 2 of 5 with total - 1 resets and a trailing write: its first
    segment reads the stored row and its last one stores, waves apart.  Its
    neighbours hold states of their own: 0 and 4 run one segment each in the
    same ticket, 1 and 3 are named by no op."""
    rng = np.random.default_rng(700 + total + fill)
    arena = rng.bytes(900)
    hs = HashStreams(eng, 5)
    ref = [Walker() for _ in range(5)]
    preload(hs, ref, rng, {0: 130, 1: fill + 1, 2: fill, 3: 128, 4: 3})
    ops = [(0, W, 0, 30), (0, S, 0, 0)]
    for k in range(total - 1):  # the first segment sums what the stored fill began
        ops += [(2, W, int(rng.integers(0, 700)), int(rng.integers(1, 200))) for _ in range(k % 3 if k else 1)]
        ops.append((2, R, 0, 0) if k % 4 == 1 else (2, SR, 0, 0))
    ops += [(2, W, 11, 175), (4, W, 30, 200), (4, S, 0, 0), (4, W, 1, 1)]
    seg_stream, _, flags, *_ = stream_seg_plan(ops, 5, 900)
    assert seg_stream.size == total + 2 and flags[1] == FIRST and flags[total] == LAST
    # FIRST in lane 1, LAST in lane `total`: in different waves from 64 on
    assert values(eng.wait(hs.submit(ops, arena))) == run_ref(ref, arena, ops)
    check_states(hs, ref)
    hs.close()


# ---- where the values land ------------------------------------------------------------------

@pytest.mark.parametrize("where", ["pinned_aligned", "pinned_offset_8", "pageable"])
def test_values_out_memory_kinds(eng, where):
    rng = np.random.default_rng(95)
    n = 6
    hs = HashStreams(eng, n)
    ref = [Walker() for _ in range(n)]
    arena = rng.bytes(1500)
    ops = random_ops(rng, n, 300, 1500, p_cut=0.3)
    k = sum(1 for op in ops if op[1] in (S, SR))
    assert k > 10
    if where == "pageable":
        out = np.zeros((k, 32), dtype=np.uint8)
    else:
        raw = eng.host_empty(32 * k + 16)
        at = 8 if where == "pinned_offset_8" else 0
        out = raw[at:at + 32 * k].reshape(k, 32)
        out[:] = 0
    t = hs.submit(ops, arena, out=out)
    assert t.values is out
    assert values(eng.wait(t)) == run_ref(ref, arena, ops)
    check_states(hs, ref)
    hs.close()


# ---- both forms on one object ---------------------------------------------------------------

def test_run_export_and_submit_mixed_without_waiting(eng):
    """run, submit, run, export_state, import_state: the library orders each
    behind the ticket in flight, the caller never waits in between."""
    rng = np.random.default_rng(94)
    n = 9
    hs = HashStreams(eng, n)
    ref = [Walker() for _ in range(n)]
    pending = []
    for step in range(4):
        arena = rng.bytes(2000)
        ops = random_ops(rng, n, 150, 2000)
        assert values(hs.run(ops, arena)) == run_ref(ref, arena, ops), step
        ops = random_ops(rng, n, 300, 2000, p_cut=0.4)
        pending.append((hs.submit(ops, arena), run_ref(ref, arena, ops)))
        ops = random_ops(rng, n, 80, 2000)
        assert values(hs.run(ops, arena)) == run_ref(ref, arena, ops), step
        assert values(hs.export_state(np.arange(n))) == [marshal_of(r.written) for r in ref], step
        if step == 2:  # import behind a ticket too
            hs.submit([(0, W, 0, 177)], arena)
            ref[0].run(W, arena[:177])
            hs.import_state([0], np.frombuffer(marshal_of(b"xyz"), dtype=np.uint8))
            ref[0] = Walker(b"xyz")
    for t, want in pending:  # values of tickets retired long ago are still theirs
        assert values(eng.wait(t)) == want
    check_states(hs, ref)
    hs.close()


# ---- tickets and the context's hasher -------------------------------------------------------

def test_a_ticket_keeps_the_function_it_was_queued_with(own):
    rng = np.random.default_rng(96)
    arena = rng.bytes(3000)
    try:
        own.set_hasher(NAME)
        hs = HashStreams(own, 8)
        ref = [Walker() for _ in range(8)]
        ops = random_ops(rng, 8, 200, 3000, p_cut=0.3)
        t = hs.submit(ops, arena)
        own.set_hasher("sha256")  # retired under SHA-256: still SHA-512/256 values
        msgs = [b"a" * 70, b"", b"abc"]
        assert values(own.hash_messages(msgs)) == [hashlib.sha256(m).digest() for m in msgs]
        assert values(own.wait(t)) == run_ref(ref, arena, ops)
        own.set_hasher(NAME)
        check_states(hs, ref)
        hs.close()
    finally:
        own.set_hasher("sha256")


def test_a_stream_ticket_beside_a_hashing_ticket(eng):
    rng = np.random.default_rng(97)
    arena = rng.bytes(4000)
    hs = HashStreams(eng, 70)
    ref = [Walker() for _ in range(70)]
    msgs = [rng.bytes(int(k)) for k in rng.integers(0, 500, 300)]
    ops = random_ops(rng, 70, 600, 4000, p_cut=0.3)
    t_hash = eng.submit_slices([[m] for m in msgs])
    t_stream = hs.submit(ops, arena)
    t_hash2 = eng.submit_slices([[m, m] for m in msgs[:50]])
    assert t_stream.value == t_hash.value + 1 and t_hash2.value == t_stream.value + 1
    assert values(eng.wait(t_hash2)) == [H(m + m) for m in msgs[:50]]
    assert values(eng.wait(t_stream)) == run_ref(ref, arena, ops)
    assert values(eng.wait(t_hash)) == [H(m) for m in msgs]
    check_states(hs, ref)
    hs.close()
