"""Host side of the mixed hash-and-verify ring submissions (no GPU):
mirsha_expect_plan through ctypes against a numpy restatement, the
``expect_plan`` helper, and Processor.submit / ProcessorWorkPool.process with
``verify_on_device=True`` over a hashlib stand-in engine that implements
``submit_slices_expect`` / ``wait``."""
import hashlib

import numpy as np
import pytest

from mirbft_amd import (Actions, HashRequest, Processor, ProcessorWorkPool, _lib, expect_bitmap, expect_plan)


# ---- mirsha_expect_plan ---------------------------------------------------------

def raw_plan(expect_of, n, m=None):
    """mirsha_expect_plan; returns (rc, has, base) with one guard entry each."""
    of = np.ascontiguousarray(expect_of, dtype=np.uint32)
    words = (n + 63) // 64
    has = np.full(words + 1, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    base = np.full(words + 1, 0xFFFFFFFF, dtype=np.uint32)
    rc = _lib.load().mirsha_expect_plan(of.ctypes.data if of.size else None, of.size if m is None else m, n,
                                        has.ctypes.data, base.ctypes.data)
    assert has[words] == np.uint64(0xFFFFFFFFFFFFFFFF) and base[words] == 0xFFFFFFFF, "wrote past its outputs"
    return rc, has[:words], base[:words]


def numpy_plan(expect_of, n):
    words = (n + 63) // 64
    flags = np.zeros(words * 64, dtype=np.uint8)
    flags[np.asarray(expect_of, dtype=np.int64)] = 1
    has = np.packbits(flags, bitorder="little").view(np.uint64)
    per_word = flags.reshape(words, 64).sum(axis=1)
    base = np.concatenate(([0], np.cumsum(per_word)[:-1])).astype(np.uint32) if words else np.zeros(0, np.uint32)
    return has, base


def masks(n):
    out = {"empty": [], "full": list(range(n)), "alternating": list(range(0, n, 2))}
    if n:
        out["first"] = [0]
        out["last"] = [n - 1]
    if n > 64:
        out["63,64"] = [63, 64]
    return out


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 128, 1000])
def test_expect_plan_matches_numpy(n):
    for name, of in masks(n).items():
        rc, has, base = raw_plan(of, n)
        assert rc == _lib.MIRSHA_OK, name
        want_has, want_base = numpy_plan(of, n)
        assert np.array_equal(has, want_has), name
        assert np.array_equal(base, want_base), name
        # the row formula: request i's expectation is row k of the m rows
        for k, i in enumerate(of):
            w, b = i >> 6, i & 63
            below = int(has[w]) & ((1 << b) - 1)
            assert int(base[w]) + bin(below).count("1") == k, (name, i)
        h2, b2 = expect_bitmap(of, n)
        assert np.array_equal(h2, want_has) and np.array_equal(b2, want_base)


@pytest.mark.parametrize("of,n,m", [
    ([3, 2], 10, None),        # not increasing
    ([2, 2], 10, None),        # a duplicate index
    ([1, 10], 10, None),       # an index == n
    ([0], 0, None),            # m > n (and an index >= n)
    ([0, 1, 2], 2, None),      # m > n
])
def test_expect_plan_rejects(of, n, m):
    rc, _, _ = raw_plan(of, n, m)
    assert rc == _lib.MIRSHA_EINVAL


def test_expect_plan_helper():
    d = [hashlib.sha256(bytes([k])).digest() for k in range(6)]
    expected = [None, d[1], d[2][:20], None, b"", bytearray(d[5])]
    of, rows, short = expect_plan(expected)
    assert of.dtype == np.uint32 and of.tolist() == [1, 2, 4, 5]
    assert rows.dtype == np.uint8 and rows.shape == (4, 32)
    assert rows[0].tobytes() == d[1] and rows[3].tobytes() == d[5]
    # a 20-byte and an empty expectation: zero rows for the device, listed by request index
    assert not rows[1].any() and not rows[2].any() and short.tolist() == [2, 4]
    of, rows, short = expect_plan([None, None])
    assert of.size == 0 and rows.shape == (0, 32) and short.size == 0
    of, rows, short = expect_plan([])
    assert of.size == 0 and rows.shape == (0, 32) and short.size == 0


# ---- Processor over a stand-in engine ----------------------------------------------

def sha(data):
    h = hashlib.sha256()
    for s in data:
        h.update(s)
    return h.digest()


class StandInTicket:
    def __init__(self, value, out, has=None, mismatches=None):
        self.value, self.out, self.has, self.mismatches = value, out, has, mismatches


class HashlibRing:
    """CPU stand-in with the ring's Python interface (submit_slices,
    submit_slices_expect, wait, poll); records every call in ``log``.  Like the
    device, a mixed submission leaves the row of a matching request unwritten
    (0xA5 here) and a wrong-length expectation is a mismatch."""

    def __init__(self):
        self.log = []
        self._next = 1

    def _ticket(self, *a):
        t = StandInTicket(self._next, *a)
        self._next += 1
        return t

    def submit_slices(self, requests, dedup=False):
        self.log.append(("submit_slices", len(requests), dedup))
        out = np.frombuffer(b"".join(sha(r) for r in requests), dtype=np.uint8).reshape(len(requests), 32)
        return self._ticket(out)

    def submit_slices_expect(self, requests, expected):
        self.log.append(("submit_slices_expect", len(requests), sum(e is not None for e in expected)))
        n = len(requests)
        out = np.full((n, 32), 0xA5, dtype=np.uint8)
        has = np.asarray([e is not None for e in expected], dtype=bool)
        bad = []
        for i, (r, e) in enumerate(zip(requests, expected)):
            d = sha(r)
            if e is not None and bytes(e) != d:
                bad.append(i)
            if e is None or bytes(e) != d:
                out[i] = np.frombuffer(d, dtype=np.uint8)
        return self._ticket(out, has, np.asarray(bad, dtype=np.int64))

    def wait(self, ticket):
        self.log.append(("wait", ticket.value))
        return ticket.out

    def poll(self, ticket):
        self.log.append(("poll", ticket.value))
        return True

    def verify_slices(self, requests, expected):
        self.log.append(("verify_slices", len(requests)))
        return np.asarray([i for i, (r, e) in enumerate(zip(requests, expected)) if sha(r) != bytes(e)],
                          dtype=np.int64)

    def hash_slices(self, requests, dedup=False):
        self.log.append(("hash_slices", len(requests)))
        return np.frombuffer(b"".join(sha(r) for r in requests), dtype=np.uint8).reshape(len(requests), 32)


def mixed_cycle(n=90):
    """Every third request carries an expectation; three are wrong, one of them in length."""
    rng = np.random.default_rng(4)
    cycle = []
    for i in range(n):
        data = [rng.integers(0, 256, int(rng.integers(0, 80)), dtype=np.uint8).tobytes()
                for _ in range(int(rng.integers(1, 4)))]
        exp = None
        if i % 3 == 0:
            exp = sha(data)
            if i in (6, 60):
                exp = bytes(32)
            if i == 33:
                exp = exp[:20]
        cycle.append(HashRequest(data, ("origin", i), exp))
    return cycle


def assert_same(results, cycle):
    assert [r.digest for r in results.digests] == [sha(r.data) for r in cycle]
    assert all(type(r.digest) is bytes and len(r.digest) == 32 for r in results.digests)
    assert all(a.request is b for a, b in zip(results.digests, cycle))  # back-pointers, origin order
    assert results.checkpoints == []


def test_submit_with_verify_is_one_mixed_submission():
    cycle = mixed_cycle()
    plain = Processor(HashlibRing()).submit(Actions(hash=cycle)).wait()
    assert_same(plain, cycle)
    ring = HashlibRing()
    pending = Processor(ring, verify_on_device=True).submit(Actions(hash=cycle))
    assert ring.log == [("submit_slices_expect", 90, 30)]
    got = pending.wait()
    assert_same(got, cycle)
    assert [r.digest for r in got.digests] == [r.digest for r in plain.digests]
    assert ring.log == [("submit_slices_expect", 90, 30), ("wait", 1)]
    assert pending.wait() is got and len(ring.log) == 2  # collected once
    # an empty cycle submits nothing
    ring = HashlibRing()
    assert Processor(ring, verify_on_device=True).submit(Actions()).wait().digests == [] and ring.log == []


def test_pool_with_verify_keeps_the_overlap():
    cycle = mixed_cycle()
    ring = HashlibRing()
    pool = ProcessorWorkPool(ring, verify_on_device=True)
    got = pool.process(Actions(hash=cycle), overlap=lambda: ring.log.append(("overlap",)))
    assert_same(got, cycle)
    # one submission, the caller's work, then the wait: no synchronous verify / hash call
    assert ring.log == [("submit_slices_expect", 90, 30), ("overlap",), ("wait", 1)]
    ring = HashlibRing()
    ProcessorWorkPool(ring).process(Actions(hash=cycle), overlap=lambda: ring.log.append(("overlap",)))
    assert ring.log == [("submit_slices", 90, False), ("overlap",), ("wait", 1)]  # the same order without the flag


def test_submit_with_verify_and_dedup_is_two_submissions():
    cycle = mixed_cycle()
    ring = HashlibRing()
    pool = ProcessorWorkPool(ring, dedup=True, verify_on_device=True)
    got = pool.process(Actions(hash=cycle), overlap=lambda: ring.log.append(("overlap",)))
    assert_same(got, cycle)
    assert ring.log == [("submit_slices_expect", 30, 30), ("submit_slices", 60, True), ("overlap",), ("wait", 1),
                        ("wait", 2)]
    # nothing carries an expectation: one dedup submission; everything does: one mixed submission
    ring = HashlibRing()
    none = [HashRequest(r.data, r.origin) for r in cycle]
    assert_same(Processor(ring, dedup=True, verify_on_device=True).submit(Actions(hash=none)).wait(), none)
    assert [e[0] for e in ring.log] == ["submit_slices", "wait"]
    ring = HashlibRing()
    every = [HashRequest(r.data, r.origin, sha(r.data)) for r in cycle]
    assert_same(Processor(ring, dedup=True, verify_on_device=True).submit(Actions(hash=every)).wait(), every)
    assert [e[0] for e in ring.log] == ["submit_slices_expect", "wait"]


def test_process_keeps_its_synchronous_split():
    cycle = mixed_cycle()
    ring = HashlibRing()
    assert_same(Processor(ring, verify_on_device=True).process(Actions(hash=cycle)), cycle)
    assert [e[0] for e in ring.log] == ["verify_slices", "hash_slices"]


def test_pending_done_polls_every_part():
    cycle = mixed_cycle(12)
    ring = HashlibRing()
    pending = Processor(ring, dedup=True, verify_on_device=True).submit(Actions(hash=cycle))
    assert pending.done()
    assert [e for e in ring.log if e[0] == "poll"] == [("poll", 1), ("poll", 2)]
