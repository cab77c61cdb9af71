"""The second hasher on the device: SHA-512/256 (sha512.New512_256 as the
Processor's `Hasher`, processor.go:21,58) through the hash, verify and ring
calls, against hashlib, bit-exact.  The shapes are the smallest at which the
two kernels of mirsha_sha512.hip can still go wrong: every padding case at
every byte alignment, tile edges, the arena's end (single-dword loads), a long
lane beside short ones, list sizes around the four-rows-a-block boundary."""
import ctypes
import hashlib

import numpy as np
import pytest

from mirbft_amd import (STREAM_SUM, STREAM_WRITE, Actions, CheckpointChains, Engine, GpuHash, HashRequest, HashStreams,
                        MirshaError, Processor, _lib, bucket_order, sharding)
from mirbft_amd.engine import KERNEL_FUSED, KERNEL_LISTS, KERNEL_MSGS

pytestmark = pytest.mark.gpu
NULL = _lib.MIRSHA_NULL_INDEX


def H(b) -> bytes:
    return hashlib.new("sha512_256", bytes(b)).digest()


def rows(digests) -> np.ndarray:
    return np.frombuffer(b"".join(digests), dtype=np.uint8).reshape(-1, 32)


def want_batch(arena, off, ln) -> np.ndarray:
    a = bytes(arena)
    return rows([H(a[int(o): int(o) + int(k)]) for o, k in zip(off, ln)])


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
    own.set_order_mode("host")
    assert own.hasher == "sha512_256"
    yield own
    own.set_hasher("sha256")


def _torch():
    import torch

    assert torch.cuda.is_available()
    return torch


def dev(a: np.ndarray):
    return _torch().from_numpy(np.ascontiguousarray(a)).cuda()


def hash_device(eng, arena: np.ndarray, off, ln, order=None) -> np.ndarray:
    """One hash_batch_device launch over an exactly sized device arena."""
    torch = _torch()
    n = len(off)
    d_arena = dev(arena if arena.size else np.zeros(1, dtype=np.uint8))
    d_off, d_len = dev(np.asarray(off, dtype=np.uint64).view(np.int64)), dev(np.asarray(ln, dtype=np.uint32).view(np.int32))
    d_order = None if order is None else dev(np.asarray(order, dtype=np.uint32).view(np.int32))
    d_out = torch.full((n, 32), 0xEE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()  # torch's stream vs the engine's own (non-blocking) stream
    eng.hash_batch_device(d_arena.data_ptr(), int(arena.size), d_off.data_ptr(), d_len.data_ptr(),
                          None if d_order is None else d_order.data_ptr(), n, d_out.data_ptr())
    eng.sync()
    return d_out.cpu().numpy()


def packed(lengths, rng, lead=0, align=None):
    """Messages of `lengths` packed behind `lead` bytes; align = (k -> offset
    mod 4) forces each message's byte alignment."""
    off, pos = [], lead
    for k, L in enumerate(lengths):
        if align is not None:
            pos += (align(k) - pos) % 4
        off.append(pos)
        pos += L
    arena = rng.integers(0, 256, size=pos, dtype=np.uint8)
    return arena, np.asarray(off, dtype=np.uint64), np.asarray(lengths, dtype=np.uint32)


# 1 ---------------------------------------------------------------------------
def test_every_padding_case_at_every_alignment(eng):
    rng = np.random.default_rng(1)
    lengths = [L for L in range(301) for _ in range(4)]
    arena, off, ln = packed(lengths, rng, align=lambda k: k % 4)
    assert sorted(set((off % 4).tolist())) == [0, 1, 2, 3] and off.size == 1204
    want = want_batch(arena, off, ln)
    assert np.array_equal(eng.hash_batch(arena, off, ln), want)
    p = rng.permutation(off.size)  # tiles now mix block counts
    assert np.array_equal(eng.hash_batch(arena, off[p], ln[p]), want[p])


# 2 ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_tile_edges_with_and_without_an_order(eng, n):
    rng = np.random.default_rng(100 + n)
    arena, off, ln = packed(rng.integers(0, 701, size=n).tolist(), rng, lead=3)
    want = want_batch(arena, off, ln)
    assert np.array_equal(hash_device(eng, arena, off, ln), want)
    order, _ = bucket_order(ln)
    assert np.array_equal(hash_device(eng, arena, off, ln, order), want)


# 3 ---------------------------------------------------------------------------
@pytest.mark.parametrize("align", [0, 1, 2, 3])
def test_last_message_ends_exactly_at_the_arena_end(eng, align):
    """The range check covers a whole access, so the arena's last block takes
    single-dword loads; a loader that used a wide load there reads zeros."""
    rng = np.random.default_rng(300 + align)
    for tail in list(range(1, 21)) + [130, 257]:
        start = 8 + align
        arena = rng.integers(1, 256, size=start + tail, dtype=np.uint8)  # no zero byte: zeros would show
        off, ln = np.array([0, start], dtype=np.uint64), np.array([5, tail], dtype=np.uint32)
        got = hash_device(eng, arena, off, ln)
        assert np.array_equal(got, want_batch(arena, off, ln)), (align, tail)


# 4 ---------------------------------------------------------------------------
def test_a_long_lane_beside_short_ones_and_one_big_message(eng):
    rng = np.random.default_rng(4)
    lengths = rng.integers(0, 201, size=64).tolist()
    lengths[17] = 70_000
    arena, off, ln = packed(lengths, rng, lead=1)
    assert np.array_equal(eng.hash_batch(arena, off, ln), want_batch(arena, off, ln))
    big = rng.integers(0, 256, size=1 << 20, dtype=np.uint8)
    assert eng.hash_batch(big, [0], [big.size])[0].tobytes() == H(big)


# 5 ---------------------------------------------------------------------------
def list_shapes(rng, n_lists, n_digests):
    sizes = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 20, 500]
    lists = []
    for k in range(n_lists):
        c = sizes[k % len(sizes)]
        ids = rng.integers(0, n_digests, size=c).tolist()
        form = (k // len(sizes)) % 6
        if form == 1:
            ids = [NULL] + ids
        elif form == 2:
            ids = ids[: c // 2] + [NULL, NULL] + ids[c // 2:]
        elif form == 3:
            ids = ids + [NULL]
        elif form == 4:
            ids = [NULL] * c
        elif form == 5:
            ids = sorted(ids, reverse=True) + ids[:1] * 3  # descending, then a repeated index
        lists.append(ids)
    return lists


@pytest.mark.parametrize("n_lists", [1, 64, 65, 257])
def test_digest_lists_host_and_device(eng, n_lists):
    torch = _torch()
    rng = np.random.default_rng(500 + n_lists)
    n_digests = 77
    table = rng.integers(0, 256, size=(n_digests, 32), dtype=np.uint8)
    lists = list_shapes(rng, n_lists, n_digests) if n_lists > 1 else [[5, NULL, 5, 76, 0]]
    idx = np.asarray([i for ids in lists for i in ids], dtype=np.uint32)
    first = np.concatenate([[0], np.cumsum([len(ids) for ids in lists])]).astype(np.uint32)
    want = rows([H(b"".join(table[i].tobytes() for i in ids if i != NULL)) for ids in lists])
    assert np.array_equal(eng.digest_lists(table, idx, first), want)
    d_table, d_first = dev(table), dev(first.view(np.int32))
    d_idx = dev((idx if idx.size else np.zeros(1, dtype=np.uint32)).view(np.int32))
    d_out = torch.full((n_lists, 32), 0xEE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    eng.digest_lists_device(d_table.data_ptr(), n_digests, d_idx.data_ptr(), d_first.data_ptr(), n_lists,
                            int(idx.size), d_out.data_ptr())
    eng.sync()
    assert np.array_equal(d_out.cpu().numpy(), want)


def test_empty_and_all_null_lists_are_the_empty_message(eng):
    table = np.zeros((1, 32), dtype=np.uint8)
    got = eng.digest_lists(table, np.array([NULL, NULL, NULL], dtype=np.uint32), np.array([0, 0, 3], dtype=np.uint32))
    assert got[0].tobytes() == got[1].tobytes() == H(b"")


# 6 ---------------------------------------------------------------------------
def test_requests_then_batches_takes_the_staged_route(eng, monkeypatch):
    monkeypatch.setenv("MIRSHA_PIPELINE_MODE", "fused")
    rng = np.random.default_rng(6)
    n = 1000
    arena, off, ln = packed([272] * n, rng)
    idx, first = sharding.batch_lists(n, 20)
    idx = idx.copy()
    idx[[0, 7, 399, 999]] = NULL
    eng.set_timing(True)
    try:
        eng.reset_timing()
        req, bat = eng.hash_requests_then_batches(arena, off, ln, idx, first)
        launches = {k: eng.kernel_time(k)[0] for k in (KERNEL_MSGS, KERNEL_LISTS, KERNEL_FUSED)}
    finally:
        eng.set_timing(False)
    want_req = want_batch(arena, off, ln)
    assert np.array_equal(req, want_req)
    want_bat = rows([H(b"".join(want_req[i].tobytes() for i in idx[first[b]: first[b + 1]] if i != NULL))
                     for b in range(first.size - 1)])
    assert np.array_equal(bat, want_bat)
    assert launches[KERNEL_MSGS] >= 1 and launches[KERNEL_LISTS] == 1 and launches[KERNEL_FUSED] == 0, launches


# 7 ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big_cycle():
    """~40 MiB: the pipelined staging route of hash_batch."""
    n, size = 131_072, 320
    arena = np.random.default_rng(7).integers(0, 256, size=n * size, dtype=np.uint8)
    off = np.arange(n, dtype=np.uint64) * size
    ln = np.full(n, size, dtype=np.uint32)
    return arena, off, ln, want_batch(arena, off, ln)


@pytest.mark.parametrize("pinned", [False, True])
def test_pipelined_staging_route(eng, big_cycle, pinned):
    arena, off, ln, want = big_cycle
    src = arena
    if pinned:
        src = eng.host_empty(arena.size)
        src[:] = arena
    assert np.array_equal(eng.hash_batch(src, off, ln), want)


# 8 ---------------------------------------------------------------------------
def test_verify_calls(eng):
    rng = np.random.default_rng(8)
    n = 200
    arena, off, ln = packed(rng.integers(0, 401, size=n).tolist(), rng)
    a = bytes(arena)
    msgs = [a[int(o): int(o) + int(k)] for o, k in zip(off, ln)]
    good = [H(m) for m in msgs]
    bad_at = [3, 64, 199]
    bad = [bytes(32) if i in bad_at else d for i, d in enumerate(good)]
    sha256 = [hashlib.sha256(m).digest() for m in msgs]
    reqs = [[m[: len(m) // 2], m[len(m) // 2:]] for m in msgs]
    for call in (lambda e: eng.verify_batch(arena, off, ln, e), lambda e: eng.verify_slices(reqs, e)):
        assert call(good).tolist() == []
        assert call(bad).tolist() == bad_at
        assert call(sha256).tolist() == list(range(n))
    table = rows(good)
    idx, first = sharding.batch_lists(n, 7)
    nl = first.size - 1
    lists = lambda h: [h(b"".join(good[i] for i in idx[first[b]: first[b + 1]])) for b in range(nl)]
    lgood = lists(H)
    lbad_at = [0, 11, nl - 1]
    lbad = [bytes(32) if b in lbad_at else d for b, d in enumerate(lgood)]
    assert eng.verify_digest_lists(table, idx, first, lgood).tolist() == []
    assert eng.verify_digest_lists(table, idx, first, lbad).tolist() == lbad_at
    assert eng.verify_digest_lists(table, idx, first, lists(lambda b: hashlib.sha256(b).digest())).tolist() == list(range(nl))


# 9 ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cycle():
    """About 300 requests of 0..400 B with duplicates and an empty request."""
    rng = np.random.default_rng(9)
    msgs = [rng.integers(0, 256, size=int(L), dtype=np.uint8).tobytes() for L in rng.integers(0, 401, size=240)]
    msgs += [msgs[k] for k in range(0, 120, 2)]  # duplicates
    msgs[5] = b""
    msgs.append(b"")
    order = rng.permutation(len(msgs))
    msgs = [msgs[k] for k in order]
    want = [H(m) for m in msgs]
    expected = [want[i] if i % 3 == 0 else None for i in range(len(msgs))]
    expected[9] = bytes(32)  # one wrong expectation
    return msgs, want, expected


def as_arena(msgs):
    ln = np.asarray([len(m) for m in msgs], dtype=np.uint32)
    off = np.concatenate([[0], np.cumsum(ln[:-1], dtype=np.uint64)]).astype(np.uint64)
    return np.frombuffer(b"".join(msgs), dtype=np.uint8), off, ln


def check_mixed(ticket, want, expected):
    assert ticket.mismatches.tolist() == [9]
    for i, e in enumerate(expected):
        if e is None or i == 9:
            assert ticket.out[i].tobytes() == want[i], i
        else:
            assert ticket.out[i].tobytes() == b"\xee" * 32, i  # a match's row is not written


def test_ring_submit_slices_plain_and_dedup(eng, cycle):
    msgs, want, _ = cycle
    reqs = [[m[:7], m[7:]] for m in msgs]
    assert np.array_equal(eng.wait(eng.submit_slices(reqs)), rows(want))
    assert np.array_equal(eng.wait(eng.submit_slices(reqs, dedup=True)), rows(want))


@pytest.mark.parametrize("pinned", [False, True])
def test_ring_submit_batch(eng, cycle, pinned):
    msgs, want, _ = cycle
    arena, off, ln = as_arena(msgs)
    out = eng.host_empty(32 * len(msgs)).reshape(-1, 32) if pinned else None
    assert np.array_equal(eng.wait(eng.submit_batch(arena, off, ln, out=out)), rows(want))


def test_ring_mixed_submissions(eng, cycle):
    msgs, want, expected = cycle
    n = len(msgs)
    arena, off, ln = as_arena(msgs)
    fill = lambda: np.full((n, 32), 0xEE, dtype=np.uint8)
    t = eng.submit_batch_expect(arena, off, ln, expected, out=fill())
    eng.wait(t)
    check_mixed(t, want, expected)
    reqs = [[m] for m in msgs]
    plain = eng.submit_slices_expect(reqs, expected, out=fill())
    eng.wait(plain)
    check_mixed(plain, want, expected)
    dd = eng.submit_slices_expect_dedup(reqs, expected, out=fill())
    eng.wait(dd)
    assert dd.n_unique == len(set(msgs))
    assert dd.mismatches.tolist() == plain.mismatches.tolist()
    assert dd.out.tobytes() == plain.out.tobytes()  # byte for byte the plain mixed submission's


def test_ring_five_submissions_reuse_slots(eng, cycle):
    msgs, want, _ = cycle
    tickets = [eng.submit_slices([[m] for m in msgs[k:]], dedup=bool(k & 1)) for k in range(5)]
    for k, t in enumerate(tickets):
        assert np.array_equal(eng.wait(t), rows(want[k:])), k


def test_ring_device_built_order(eng):
    rng = np.random.default_rng(10)
    arena, off, ln = packed(rng.integers(0, 701, size=300).tolist(), rng)
    eng.set_order_mode("device")
    try:
        got = eng.wait(eng.submit_batch(arena, off, ln))
    finally:
        eng.set_order_mode("host")
    assert np.array_equal(got, want_batch(arena, off, ln))


# 10 --------------------------------------------------------------------------
def test_processor_with_the_second_hasher(own, cycle):
    msgs, want, expected = cycle
    own.set_hasher("sha256")
    try:
        p = Processor(engine=own, hasher="sha512_256", dedup=True, verify_on_device=True)
        assert own.hasher == "sha512_256"
        reqs = [HashRequest(data=[m[:3], m[3:]], origin=i, expected=e) for i, (m, e) in enumerate(zip(msgs, expected))]
        for results in (p.process(Actions(hash=reqs)), p.submit(Actions(hash=reqs)).wait()):
            # the loop of processor.go:133-143 restated: Digests[i] for actions.Hash[i], back-pointers kept
            assert [r.request for r in results.digests] == reqs
            assert [bytes(r.digest) for r in results.digests] == want
        g = GpuHash(own)
        g.write(b"ab")
        g.write(b"c")
        assert g.sum() == H(b"abc") and g.sum(b"x") == b"x" + H(b"abc")
        assert (g.size, g.block_size) == (32, 128)
    finally:
        own.set_hasher("sha256")
    assert (GpuHash(own).size, GpuHash(own).block_size) == (32, 64)


# 11 --------------------------------------------------------------------------
def test_default_untouched_and_refusals_loud(own):
    msgs = [b"", b"abc", b"x" * 200, b"y" * 129]
    sha256 = rows([hashlib.sha256(m).digest() for m in msgs])
    own.set_hasher("sha256")
    table = np.arange(64, dtype=np.uint8).reshape(2, 32)
    ops = ([0, 0, 0], [0, 1, _lib.MIRSHA_COMMIT_CHECKPOINT])
    chains, streams = CheckpointChains(own, 2), HashStreams(own, 1)
    try:
        assert np.array_equal(own.hash_messages(msgs), sha256)
        own.set_hasher("sha512_256")
        assert np.array_equal(own.hash_messages(msgs), rows([H(m) for m in msgs]))
        idx, first = sharding.batch_lists(4, 2)
        for refused in (lambda: chains.commit(table, *ops),
                        lambda: streams.run([(0, STREAM_WRITE, 0, 3), (0, STREAM_SUM)], b"abc"),
                        lambda: own.pipeline(4, idx, first, np.full(4, 8, dtype=np.uint32))):
            with pytest.raises(MirshaError) as ei:
                refused()
            assert ei.value.code == _lib.MIRSHA_EINVAL and "sha512_256" in str(ei.value), str(ei.value)
        ticket = own.submit_slices([[m] for m in msgs])  # queued under SHA-512/256 ...
        own.set_hasher("sha256")
        assert np.array_equal(own.wait(ticket), rows([H(m) for m in msgs]))  # ... and it stays that
        assert np.array_equal(own.hash_messages(msgs), sha256)
        # the refused calls changed nothing: the same objects give what they would have given
        assert chains.commit(table, *ops)[0].tobytes() == hashlib.sha256(table.tobytes()).digest()
        assert streams.run([(0, STREAM_WRITE, 0, 3), (0, STREAM_SUM)], b"abc")[0].tobytes() == hashlib.sha256(b"abc").digest()
        with pytest.raises(MirshaError) as ei:
            own._check(own._lib.mirsha_ctx_set_hasher(own.ctx, 7))
        assert ei.value.code == _lib.MIRSHA_EINVAL and own.hasher == "sha256"
    finally:
        own.set_hasher("sha256")
        chains.close()
        streams.close()


def test_hash_batch_device_refuses_more_than_one_descriptor(eng):
    """No 64-bit-addressed SHA-512 form: MIRSHA_ERANGE ahead of any launch (the
    pointers are never read)."""
    for arena_len, n in ((0xFFFFFF01, 1), (64, 1 << 27)):
        with pytest.raises(MirshaError) as ei:
            eng.hash_batch_device(16, arena_len, 16, 16, None, n, 16)
        assert ei.value.code == _lib.MIRSHA_ERANGE


# 12 --------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [8, 8 | 1, 8 | 2])
def test_cpp_mirror_with_the_second_hasher(flags):
    host = ctypes.CDLL(_lib.HOST_LIB_PATH)
    msgs = [b"m" * (i % 7) * 50 for i in range(100)]
    bufs = [ctypes.create_string_buffer(m, len(m) or 1) for m in msgs]
    data = (ctypes.c_void_p * len(msgs))(*[ctypes.addressof(b) for b in bufs])
    lens = (ctypes.c_uint64 * len(msgs))(*[len(m) for m in msgs])
    out = (ctypes.c_uint8 * (32 * len(msgs)))()
    err = ctypes.create_string_buffer(256)
    host.mirbft_host_process_ex.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32,
                                            ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_char_p,
                                            ctypes.c_uint32]
    rc = host.mirbft_host_process_ex(0, data, lens, len(msgs), out, flags, None, err, 256)
    assert rc == 0, err.value
    assert [bytes(out[32 * i: 32 * i + 32]) for i in range(len(msgs))] == [H(m) for m in msgs]
