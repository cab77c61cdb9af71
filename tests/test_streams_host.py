"""Host side of the streaming hash states, no GPU: mirsha_stream_plan (the
arrays mirsha_streams_run / _run_device send to the device) through ctypes
against a short Python restatement, its error codes with the offending op, and
the 108-byte state layout (Go 1.14 crypto/sha256 MarshalBinary) built by hand."""
import ctypes
import hashlib
import struct

import numpy as np
import pytest

from mirbft_amd import (STREAM_RESET, STREAM_SUM, STREAM_SUM_RESET, STREAM_WRITE, MirshaError, _lib, stream_plan)
from mirbft_amd.engine import _stream_ops

H0 = (0x6A09E667, 0xBB67AE85, 0x3C6EF372, 0xA54FF53A, 0x510E527F, 0x9B05688C, 0x1F83D9AB, 0x5BE0CD19)


def restate(ops, n_streams, pack):
    """The plan in plain Python: entries grouped by stream (ascending), in op
    order, zero-length writes dropped, value rows counted in op order."""
    per = {}
    rows = 0
    for s, kind, off, ln in ops:
        if kind == STREAM_WRITE:
            if ln:
                per.setdefault(s, []).append([kind, off, ln])
            continue
        word = kind
        if kind in (STREAM_SUM, STREAM_SUM_RESET):
            word |= rows << 2
            rows += 1
        per.setdefault(s, []).append([word, 0, 0])
    act = sorted(per)
    efirst, ent = [0], []
    for s in act:
        ent += per[s]
        efirst.append(len(ent))
    total, seen = 0, {}
    for e in ent:
        if not pack:
            total += e[2]
        elif e[2]:  # every distinct (off, len) range once, in the order of its first entry
            if (e[1], e[2]) not in seen:
                seen[e[1], e[2]] = total
                total += e[2]
            e[1] = seen[e[1], e[2]]
    return act, efirst, [e[0] for e in ent], [e[1] for e in ent], [e[2] for e in ent], rows, total


def check(ops, n_streams, arena_len):
    ops = [tuple(op) + (0, 0) * (len(op) == 2) for op in ops]
    for pack in (False, True):
        got = stream_plan(ops, n_streams, arena_len, pack=pack)
        want = restate(ops, n_streams, pack)
        assert [list(map(int, g)) for g in got[:5]] == [list(w) for w in want[:5]], (pack, ops)
        assert got[5:] == want[5:], (pack, ops)
    return got


def test_op_order_programmes_with_interleaved_streams():
    ops = [(2, STREAM_WRITE, 10, 5), (0, STREAM_WRITE, 0, 3), (2, STREAM_SUM), (0, STREAM_WRITE, 3, 7), (2, STREAM_WRITE, 1, 64),
           (0, STREAM_SUM_RESET), (2, STREAM_RESET), (0, STREAM_WRITE, 90, 10), (2, STREAM_SUM), (5, STREAM_SUM)]
    act, efirst, kind, off, ln, nv, nb = check(ops, 6, 100)
    assert act.tolist() == [0, 2, 5] and efirst.tolist() == [0, 4, 9, 10]
    # value rows in op order across the streams: stream 2's first sum is row 0, stream 0's checkpoint row 1, ...
    assert [int(k) >> 2 for k in kind if int(k) & 3 in (STREAM_SUM, STREAM_SUM_RESET)] == [1, 0, 2, 3]
    assert nv == 4 and nb == 5 + 3 + 7 + 64 + 10


def test_packed_offsets_follow_entry_order_without_gaps():
    ops = [(1, STREAM_WRITE, 50, 4), (0, STREAM_WRITE, 20, 6), (1, STREAM_WRITE, 0, 2)]
    _, _, _, off, ln, _, nb = stream_plan(ops, 2, 60, pack=True)
    assert off.tolist() == [0, 6, 10] and ln.tolist() == [6, 4, 2] and nb == 12
    assert stream_plan(ops, 2, 60)[3].tolist() == [20, 50, 0]


def test_ranges_named_again_share_their_packed_bytes():
    """N nodes applying the same log entry: its bytes cross PCIe once."""
    ops = [(s, STREAM_WRITE, off, ln) for off, ln in ((40, 8), (0, 32), (40, 9)) for s in range(3)]
    ops += [(1, STREAM_WRITE, 40, 8)]
    _, _, _, off, ln, _, nb = check(ops, 3, 60)
    assert nb == 8 + 32 + 9 and off.tolist() == [0, 8, 40, 0, 8, 40, 0, 0, 8, 40]
    assert stream_plan(ops, 3, 60)[6] == 3 * 49 + 8


def test_zero_length_writes_are_dropped_and_do_not_activate_a_stream():
    ops = [(3, STREAM_WRITE, 5, 0), (1, STREAM_WRITE, 0, 0), (1, STREAM_WRITE, 0, 4), (1, STREAM_WRITE, 10, 0), (1, STREAM_SUM),
           (3, STREAM_WRITE, 10, 0)]
    act, efirst, kind, off, ln, nv, nb = check(ops, 4, 10)
    assert act.tolist() == [1] and efirst.tolist() == [0, 2] and ln.tolist() == [4, 0] and nv == 1 and nb == 4
    # nothing but zero-length writes: no active stream at all
    act, efirst, *_ = check([(0, STREAM_WRITE, 0, 0), (2, STREAM_WRITE, 3, 0)], 3, 3)
    assert act.size == 0 and efirst.tolist() == [0]


def test_random_programmes_against_the_restatement():
    rng = np.random.default_rng(5)
    for _ in range(50):
        n_streams = int(rng.integers(1, 9))
        arena_len = int(rng.integers(0, 300))
        ops = []
        for _ in range(int(rng.integers(0, 40))):
            s = int(rng.integers(0, n_streams))
            kind = int(rng.integers(0, 4))
            if kind == STREAM_WRITE:
                off = int(rng.integers(0, arena_len + 1))
                ops.append((s, kind, off, int(rng.integers(0, arena_len - off + 1))))
            else:
                ops.append((s, kind, int(rng.integers(0, 1 << 40)), int(rng.integers(0, 1 << 32))))  # ignored
        got = check([op if op[1] == STREAM_WRITE else (op[0], op[1], 0, 0) for op in ops], n_streams, arena_len)
        # off / len of a non-write op are ignored (check() returns its packed plan)
        raw = stream_plan(ops, n_streams, arena_len, pack=True)
        assert all(np.array_equal(a, b) for a, b in zip(raw[:5], got[:5])) and raw[5:] == got[5:]


@pytest.mark.parametrize("ops,bad", [
    ([(0, STREAM_SUM), (4, STREAM_WRITE, 0, 1)], 1),                    # stream id >= n_streams
    ([(0, STREAM_SUM), (1, STREAM_RESET), (2, 4, 0, 0)], 2),             # unknown kind
    ([(0, STREAM_WRITE, 90, 11)], 0),                                    # op_off + op_len > arena_len
    ([(0, STREAM_WRITE, 0, 100), (1, STREAM_WRITE, 101, 0)], 1),         # a zero-length write past the end
    ([(0, STREAM_WRITE, (1 << 64) - 1, 2)], 0),                          # the sum must not wrap
    ([(3, STREAM_SUM), (0xFFFFFFFF, STREAM_SUM)], 1),
    ([(0, STREAM_WRITE, 0, 100), (9, 7, 0, 0), (0, STREAM_WRITE, 200, 1)], 1),  # the FIRST offending op
])
def test_every_einval_names_its_op(ops, bad):
    with pytest.raises(MirshaError) as e:
        stream_plan(ops, 4, 100)
    assert e.value.code == _lib.MIRSHA_EINVAL and e.value.bad_op == bad


def test_null_arrays_and_the_empty_programme():
    lib = _lib.load()
    n = [ctypes.c_uint32(7) for _ in range(4)]
    nb = ctypes.c_uint64(7)
    ef = np.full(1, 9, dtype=np.uint32)
    counts = (ctypes.byref(n[0]), ctypes.byref(n[1]), ctypes.byref(n[2]), ctypes.byref(nb), ctypes.byref(n[3]))
    # n_ops == 0 is valid: nothing active, efirst[0] = 0
    assert lib.mirsha_stream_plan(None, None, None, None, 0, 4, 0, 0, None, ef.ctypes.data, None, None, None,
                                  *counts) == _lib.MIRSHA_OK
    assert [x.value for x in n[:3]] == [0, 0, 0] and nb.value == 0 and ef[0] == 0 and n[3].value == 0xFFFFFFFF
    os_, ok, oo, ol = _stream_ops([(0, STREAM_WRITE, 0, 1)])
    out = np.zeros(4, dtype=np.uint64)
    p = out.ctypes.data
    # NULL op arrays, NULL output arrays, NULL counts
    assert lib.mirsha_stream_plan(None, ok.ctypes.data, oo.ctypes.data, ol.ctypes.data, 1, 4, 8, 0, p, p, p, p, p,
                                  *counts) == _lib.MIRSHA_EINVAL
    assert lib.mirsha_stream_plan(os_.ctypes.data, ok.ctypes.data, None, ol.ctypes.data, 1, 4, 8, 0, p, p, p, p, p,
                                  *counts) == _lib.MIRSHA_EINVAL
    assert lib.mirsha_stream_plan(os_.ctypes.data, ok.ctypes.data, oo.ctypes.data, ol.ctypes.data, 1, 4, 8, 0, p, p, None,
                                  p, p, *counts) == _lib.MIRSHA_EINVAL
    assert lib.mirsha_stream_plan(os_.ctypes.data, ok.ctypes.data, oo.ctypes.data, ol.ctypes.data, 1, 4, 8, 0, p, p, p, p,
                                  p, None, *counts[1:]) == _lib.MIRSHA_EINVAL
    # a programme without writes needs no offsets and lengths
    os_, ok, _, _ = _stream_ops([(1, STREAM_SUM)])
    assert lib.mirsha_stream_plan(os_.ctypes.data, ok.ctypes.data, None, None, 1, 4, 0, 0, p, p, p, p, p,
                                  *counts) == _lib.MIRSHA_OK
    assert n[0].value == 1 and n[2].value == 1
    assert lib.mirsha_stream_plan(os_.ctypes.data, ok.ctypes.data, None, None, _lib.MIRSHA_STREAM_MAX_OPS + 1, 4, 0, 0,
                                  p, p, p, p, p, *counts) == _lib.MIRSHA_ERANGE


def marshal(h, buffered: bytes, length: int) -> bytes:
    """Go 1.14 crypto/sha256 (*digest).MarshalBinary, by its description: the
    magic, h[0..7] big-endian, the buffer zero-padded to 64, the length."""
    assert len(buffered) == length % 64
    return b"sha\x03" + struct.pack(">8I", *h) + buffered.ljust(64, b"\0") + struct.pack(">Q", length)


def test_state_layout_by_hand():
    fresh = marshal(H0, b"", 0)
    assert len(fresh) == _lib.MIRSHA_STREAM_STATE_BYTES == 108
    assert fresh[:4] == bytes([0x73, 0x68, 0x61, 0x03]) and fresh[4:8] == bytes.fromhex("6a09e667")
    assert fresh[36:100] == bytes(64) and fresh[100:] == bytes(8)
    s = marshal(H0, b"abc", 3)
    assert s[36:39] == b"abc" and s[39:100] == bytes(61) and s[100:] == bytes(7) + b"\x03"
    assert hashlib.sha256(b"abc").digest_size * 8 == 256  # the oracle the GPU tests compare with
