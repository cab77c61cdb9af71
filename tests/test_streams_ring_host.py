"""Host side of the streams' ring form, no GPU: mirsha_stream_seg_plan (the
segments mirsha_streams_submit sends to the device) through ctypes against a
short Python restatement, and the algebra the segment kernel rests on, against
hashlib: every segment hashed by an object of its own gives the values and the
leftover state of the sequential walk."""
import ctypes
import hashlib

import numpy as np
import pytest

from mirbft_amd import (STREAM_RESET, STREAM_SUM, STREAM_SUM_RESET, STREAM_WRITE, MirshaError, _lib, stream_plan,
                        stream_seg_plan)
from mirbft_amd.engine import _stream_ops
from streamref import CUTS, Walker, marshal_of, sha256_by_hand

FIRST, LAST = _lib.MIRSHA_STREAM_SEG_FIRST, _lib.MIRSHA_STREAM_SEG_LAST
W, S, SR, R = STREAM_WRITE, STREAM_SUM, STREAM_SUM_RESET, STREAM_RESET


def restate(ops):
    """The segments in plain Python, from the ops directly: per stream
    (ascending) its entries in op order, zero-length writes dropped, cut after
    every SUM_RESET / RESET; no empty segment behind a final one."""
    per = {}
    for s, kind, _, ln in ops:
        if kind == STREAM_WRITE and not ln:
            continue
        per.setdefault(s, []).append(kind)
    seg_stream, sfirst, flags, at = [], [0], [], 0
    for s in sorted(per):
        kinds = per[s]
        first = True
        for k, kind in enumerate(kinds):
            at += 1
            last = k + 1 == len(kinds)
            if kind in CUTS or last:
                seg_stream.append(s)
                flags.append((FIRST if first else 0) | (LAST if last else 0))
                sfirst.append(at)
                first = False
    return seg_stream, sfirst, flags


def check(ops, n_streams, arena_len):
    ops = [tuple(op) + (0, 0) * (len(op) == 2) for op in ops]
    for pack in (False, True):
        got = stream_seg_plan(ops, n_streams, arena_len, pack=pack)
        plan = stream_plan(ops, n_streams, arena_len, pack=pack)
        # the entry arrays and the counts are mirsha_stream_plan's own, for either value of pack
        assert all(np.array_equal(a, b) for a, b in zip(got[3:6], plan[2:5])), (pack, ops)
        assert got[6:8] == plan[5:7] and got[8] == plan[0].size, (pack, ops)
        want = restate(ops)
        assert [list(map(int, g)) for g in got[:3]] == [list(w) for w in want], (pack, ops)
        seg_stream, sfirst, flags, kind = got[0], got[1], got[2], got[3]
        assert int(sfirst[-1]) == kind.size
        # n_seg = active streams + reset-kind entries that are not their stream's final entry
        inner = 0
        for k in range(plan[0].size):
            inner += sum(1 for e in range(int(plan[1][k]), int(plan[1][k + 1]) - 1) if int(kind[e]) & 3 in CUTS)
        assert seg_stream.size == plan[0].size + inner, (pack, ops)
        for s in range(seg_stream.size):
            assert sfirst[s + 1] > sfirst[s], "an empty segment"
            assert all(int(k) & 3 not in CUTS for k in kind[int(sfirst[s]):int(sfirst[s + 1]) - 1])
            assert int(kind[int(sfirst[s + 1]) - 1]) & 3 in CUTS or flags[s] & LAST
    return got


def test_a_stream_ending_in_a_reset_gets_no_empty_segment():
    seg_stream, sfirst, flags, *_ = check([(0, W, 0, 5), (0, SR), (0, W, 5, 3), (0, R)], 1, 8)
    assert seg_stream.tolist() == [0, 0] and sfirst.tolist() == [0, 2, 4] and flags.tolist() == [FIRST, LAST]
    seg_stream, sfirst, flags, *_ = check([(1, W, 0, 5), (1, SR)], 2, 8)
    assert seg_stream.tolist() == [1] and sfirst.tolist() == [0, 2] and flags.tolist() == [FIRST | LAST]


def test_consecutive_resets_are_one_segment_each():
    seg_stream, sfirst, flags, *_ = check([(0, SR), (0, SR), (0, R), (0, R), (0, S)], 1, 0)
    assert sfirst.tolist() == [0, 1, 2, 3, 4, 5] and flags.tolist() == [FIRST, 0, 0, 0, LAST]


def test_a_lone_reset():
    seg_stream, sfirst, flags, *_ = check([(2, R)], 3, 0)
    assert seg_stream.tolist() == [2] and sfirst.tolist() == [0, 1] and flags.tolist() == [FIRST | LAST]


def test_only_zero_length_writes_plan_no_segment():
    got = check([(0, W, 0, 0), (2, W, 3, 0)], 3, 3)
    assert got[0].size == 0 and got[1].tolist() == [0] and got[8] == 0
    got = check([], 3, 3)
    assert got[0].size == 0 and got[1].tolist() == [0]


def test_a_plain_sum_does_not_cut():
    seg_stream, sfirst, flags, *_ = check([(0, W, 0, 4), (0, S), (0, W, 4, 4), (0, S), (0, SR), (0, W, 0, 1), (0, S)],
                                          1, 8)
    assert sfirst.tolist() == [0, 5, 7] and flags.tolist() == [FIRST, LAST]


def test_segments_are_stream_major_in_op_order():
    ops = [(2, W, 0, 1), (0, SR), (2, SR), (0, W, 1, 1), (2, W, 2, 1), (0, R), (1, S), (2, S)]
    seg_stream, sfirst, flags, kind, *_ = check(ops, 3, 3)
    assert seg_stream.tolist() == [0, 0, 1, 2, 2]
    assert sfirst.tolist() == [0, 1, 3, 4, 6, 8]
    assert flags.tolist() == [FIRST, LAST, FIRST | LAST, FIRST, LAST]


def random_programme(rng, n_streams, arena_len, n_ops):
    ops = []
    for _ in range(n_ops):
        s = int(rng.integers(0, n_streams))
        kind = int(rng.integers(0, 4))
        if kind == STREAM_WRITE:
            off = int(rng.integers(0, arena_len + 1))
            ops.append((s, kind, off, int(rng.integers(0, min(arena_len - off, 150) + 1))))
        else:
            ops.append((s, kind, 0, 0))
    return ops


def test_random_programmes_against_the_restatement():
    rng = np.random.default_rng(81)
    for _ in range(60):
        n_streams = int(rng.integers(1, 9))
        arena_len = int(rng.integers(0, 300))
        check(random_programme(rng, n_streams, arena_len, int(rng.integers(0, 60))), n_streams, arena_len)


@pytest.mark.parametrize("ops,bad", [
    ([(0, S), (4, W, 0, 1)], 1),
    ([(0, S), (1, R), (2, 4, 0, 0)], 2),
    ([(0, W, 90, 11)], 0),
    ([(0, W, 0, 100), (9, 7, 0, 0), (0, W, 200, 1)], 1),
])
def test_error_codes_and_bad_op_are_the_stream_plans(ops, bad):
    with pytest.raises(MirshaError) as e:
        stream_seg_plan(ops, 4, 100)
    assert e.value.code == _lib.MIRSHA_EINVAL and e.value.bad_op == bad
    with pytest.raises(MirshaError) as e2:
        stream_plan(ops, 4, 100)
    assert (e2.value.code, e2.value.bad_op) == (e.value.code, e.value.bad_op)


def test_null_arrays_and_the_op_limit():
    lib = _lib.load()
    n = [ctypes.c_uint32(7) for _ in range(5)]
    nb = ctypes.c_uint64(7)
    counts = (ctypes.byref(n[0]), ctypes.byref(n[1]), ctypes.byref(n[2]), ctypes.byref(n[3]), ctypes.byref(nb),
              ctypes.byref(n[4]))
    assert lib.mirsha_stream_seg_plan(None, None, None, None, 0, 4, 0, 0, None, None, None, None, None, None,
                                      *counts) == _lib.MIRSHA_OK
    assert [x.value for x in n[:4]] == [0, 0, 0, 0] and n[4].value == 0xFFFFFFFF
    os_, ok, oo, ol = _stream_ops([(0, W, 0, 1), (9, S, 0, 0)])
    buf = np.zeros(8, dtype=np.uint64)
    p = buf.ctypes.data
    args = (os_.ctypes.data, ok.ctypes.data, oo.ctypes.data, ol.ctypes.data, 2, 4, 8, 0)
    # a NULL output array: the plan's own checks come first (the bad op is named), else EINVAL
    assert lib.mirsha_stream_seg_plan(*args, None, p, p, p, p, p, *counts) == _lib.MIRSHA_EINVAL and n[4].value == 1
    os_[1] = 1
    for hole in range(6):
        outs = [p] * 6
        outs[hole] = None
        assert lib.mirsha_stream_seg_plan(*args, *outs, *counts) == _lib.MIRSHA_EINVAL, hole
        assert n[0].value == 0 and n[4].value == 0xFFFFFFFF
    assert lib.mirsha_stream_seg_plan(*args, p, p, p, p, p, p, None, *counts[1:]) == _lib.MIRSHA_EINVAL
    assert lib.mirsha_stream_seg_plan(*args[:4], _lib.MIRSHA_STREAM_MAX_OPS + 1, 4, 8, 0, p, p, p, p, p, p,
                                      *counts) == _lib.MIRSHA_ERANGE
    assert n[0].value == 0


# ---- the algebra: segments hashed apart = the sequential walk -----------------------------------

def test_plain_python_compression_is_sha256():
    data = bytes(range(256)) * 2
    for n in (0, 3, 55, 56, 64, 200):
        assert sha256_by_hand(data[:n]) == hashlib.sha256(data[:n]).digest()


def test_segments_hashed_apart_give_the_sequential_walk():
    rng = np.random.default_rng(82)
    for _ in range(40):
        n_streams = int(rng.integers(1, 6))
        arena = rng.bytes(int(rng.integers(1, 400)))
        stored = [rng.bytes(int(rng.integers(0, 200))) for _ in range(n_streams)]  # what each stream holds
        ops = random_programme(rng, n_streams, len(arena), int(rng.integers(1, 80)))
        # the sequential walk: one object per stream, in op order
        seq = [Walker(w) for w in stored]
        want = [v for s, kind, off, ln in ops for v in [seq[s].run(kind, arena[off:off + ln])] if v is not None]
        # the segments: one object each; FIRST starts from the stored state, every other from Hasher()
        seg_stream, sfirst, flags, kind, off, ln, nv, _, _ = stream_seg_plan(ops, n_streams, len(arena))
        got = [None] * nv
        left = {s: Walker(w) for s, w in enumerate(stored)}  # streams no segment names keep their state
        for k in range(seg_stream.size):
            s = int(seg_stream[k])
            lane = Walker(stored[s]) if flags[k] & FIRST else Walker()
            for e in range(int(sfirst[k]), int(sfirst[k + 1])):
                v = lane.run(int(kind[e]) & 3, arena[int(off[e]):int(off[e]) + int(ln[e])])
                if v is not None:
                    got[int(kind[e]) >> 2] = v
            if flags[k] & LAST:
                left[s] = lane
        assert got == want and len(want) == nv
        assert [marshal_of(left[s].written) for s in range(n_streams)] == [marshal_of(w.written) for w in seq]
        assert all(len(marshal_of(w.written)) == _lib.MIRSHA_STREAM_STATE_BYTES for w in seq)
