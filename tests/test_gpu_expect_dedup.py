"""One ring ticket for a deduplicated cycle that carries expectations
(mirsha_submit_slices_expect_dedup / mirsha_hash_slices_expect_dedup,
expect_select_gather_kernel): every distinct content is hashed once, with or
without an expectation, and the select kernel reads request i's digest from the
row of its representative and compares it with request i's own expectation.
Verdict, count and every output byte must equal those of
mirsha_submit_slices_expect on the same input, and hashlib's.

Every output is pre-filled: digests_out with 0xA5 plus one guard row, the
bitmap with 0xFF plus one guard word, the count and n_unique with 0xDEADBEEF."""
import ctypes
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from mirbft_amd import (Actions, CheckpointChains, ExpectTicket, HashRequest, Processor, SliceArrays, _lib, dedup_rows,
                        expect_plan)

pytestmark = pytest.mark.gpu

ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
SENTINEL = 0xDEADBEEF
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _p(a):
    return a.ctypes.data if a is not None and a.size else None


def sha(parts):
    return hashlib.sha256(b"".join(parts)).digest()


def digests_of(reqs):
    return np.frombuffer(b"".join(sha(r) for r in reqs), dtype=np.uint8).reshape(len(reqs), 32)


def wrong_row(row, k=0):
    bad = bytearray(row.tobytes() if isinstance(row, np.ndarray) else row)
    bad[k % 32] ^= 0x40
    return bytes(bad)


class Run:
    """One raw mirsha_submit_slices_expect[_dedup] call with pre-filled
    outputs; keeps every array the library reads or writes alive.  An
    expectation that is not 32 bytes long travels as 32 zero bytes
    (``expect_plan``), which no digest here equals: a mismatch on the device too."""

    def __init__(self, engine, reqs, expected, out=None):
        self.engine, self.reqs, self.expected = engine, reqs, list(expected)
        self.n = n = len(self.expected)
        self.of, self.rows, self.short = expect_plan(self.expected)
        self.words = (n + 63) // 64
        self.out = np.empty((n + 1, 32), dtype=np.uint8) if out is None else out
        assert self.out.shape == (n + 1, 32)
        self.out[:] = 0xA5
        self.bits = np.full(self.words + 1, ONES, dtype=np.uint64)
        self.count = np.full(1, SENTINEL, dtype=np.uint32)
        self.unique = np.full(1, SENTINEL, dtype=np.uint32)
        self.ticket = ctypes.c_uint64(0)
        self.sl = reqs if isinstance(reqs, SliceArrays) else SliceArrays.from_requests(reqs)

    def dedup(self, of=None, rows_p="own", m=None, count_p="own"):
        """The new entry; the keyword arguments replace single arguments (refusals)."""
        of = self.of if of is None else np.asarray(of, dtype=np.uint32)
        self.keep = of
        sl = self.sl
        return self.engine._lib.mirsha_submit_slices_expect_dedup(
            self.engine.ctx, sl.ptr_p, sl.len_p, sl.first_p, sl.n, _p(of), _p(self.rows) if rows_p == "own" else rows_p,
            of.size if m is None else m, self.out.ctypes.data, self.bits.ctypes.data,
            self.count.ctypes.data if count_p == "own" else count_p,
            self.unique.ctypes.data_as(_lib._u32p), ctypes.byref(self.ticket))

    def mixed(self):
        """mirsha_submit_slices_expect, flags 0: the reference submission."""
        sl = self.sl
        return self.engine._lib.mirsha_submit_slices_expect(
            self.engine.ctx, sl.ptr_p, sl.len_p, sl.first_p, sl.n, _p(self.of), _p(self.rows), self.of.size,
            self.out.ctypes.data, self.bits.ctypes.data, self.count.ctypes.data, 0, ctypes.byref(self.ticket))

    def wait(self):
        assert self.engine._lib.mirsha_wait(self.engine.ctx, self.ticket.value) == 0
        return self

    def untouched(self):
        return int(self.count[0]) == SENTINEL and bool((self.out == 0xA5).all()) and bool((self.bits == ONES).all())

    def check(self, want):
        """The whole contract of a retired ticket against the hashlib digests."""
        n = self.n
        has = np.asarray([e is not None for e in self.expected], dtype=bool)
        wrong = np.zeros(n, dtype=bool)
        for i in np.flatnonzero(has):
            wrong[i] = bytes(self.expected[i]) != want[i].tobytes()
        flags = np.zeros(self.words * 64, dtype=np.uint8)
        flags[:n] = wrong
        ref_bits = np.packbits(flags, bitorder="little").view(np.uint64)
        assert self.bits[self.words] == ONES, "wrote past the bitmap"
        assert np.array_equal(self.bits[:self.words], ref_bits)  # zero bits beyond n included
        assert int(self.count[0]) == int(wrong.sum())
        keep = ~has | wrong
        assert np.array_equal(self.out[:n][keep], want[keep]), "kept rows differ from hashlib"
        assert (self.out[:n][~keep] == 0xA5).all(), "a matching request's row was written"
        assert (self.out[n] == 0xA5).all(), "wrote past the digest rows"
        return wrong


def same_outputs(a, b):
    assert np.array_equal(a.bits, b.bits) and int(a.count[0]) == int(b.count[0])
    assert np.array_equal(a.out, b.out)  # every byte: kept rows, untouched rows, guard row


# ---- the main case -----------------------------------------------------------------

N = 131  # three bitmap words, the last one partial


def pool9():
    rng = np.random.default_rng(9)
    blob = lambda k: rng.integers(0, 256, k, dtype=np.uint8).tobytes()
    single = [[blob(k)] for k in (0, 1, 55, 56, 64, 119, 600)]  # the padding boundaries of one and two blocks
    multi = [[blob(30), b"", blob(70)], [blob(7), blob(64), blob(1), blob(200)]]
    return single + multi


def content_of(i):
    return (i + i // 9) % 9  # every nine consecutive requests hold every content once


@pytest.fixture(scope="module")
def main_case():
    """(requests, hashlib digests, expectations, the wrong indices by name)."""
    pool = pool9()
    reqs = [pool[content_of(i)] for i in range(N)]
    assert len({b"".join(r) for r in reqs}) == 9
    # every content's copies spread over the words: each has copies in both full
    # words, and the partial word's three lanes gather three further contents' rows
    for c in range(9):
        assert {i >> 6 for i in range(N) if content_of(i) == c} >= {0, 1}
    assert len({content_of(i) for i in range(128, N)}) == 3
    want = digests_of(reqs)
    want.setflags(write=False)
    expected = [want[i].tobytes() if i % 3 == 0 else None for i in range(N)]
    holders = lambda c: [i for i in range(N) if i % 3 == 0 and content_of(i) == c]
    first = lambda c: next(i for i in range(N) if content_of(i) == c)
    # content 0: the representative (request 0) is right, a duplicate is wrong
    a = holders(0)
    assert a[0] == first(0) == 0 and len(a) >= 2
    # content 3: the representative (request 3) is wrong, its duplicates are right
    b = holders(3)
    assert b[0] == first(3) == 3 and len(b) >= 2
    # content 6: two duplicates with two different wrong rows, the representative right
    c = holders(6)
    assert c[0] == first(6) == 6 and len(c) >= 3
    # content 1: its representative carries no expectation; a duplicate's is 20 bytes long
    d = holders(1)
    assert first(1) == 1 and d
    wrong = {"dup": a[-1], "rep": b[0], "two_a": c[1], "two_b": c[-1], "short": d[len(d) // 2]}
    expected[wrong["dup"]] = wrong_row(want[0])
    expected[wrong["rep"]] = wrong_row(want[3], 31)
    expected[wrong["two_a"]] = wrong_row(want[6], 5)
    expected[wrong["two_b"]] = wrong_row(want[6], 17)
    expected[wrong["short"]] = want[1].tobytes()[:20]
    assert len(set(wrong.values())) == 5 and {i >> 6 for i in wrong.values()} == {0, 1}
    return reqs, want, expected, wrong


@pytest.mark.parametrize("where", ["pageable", "page_locked"])
def test_main_case_equals_the_mixed_submission_and_hashlib(engine, main_case, where):
    reqs, want, expected, wrong = main_case
    outs = [None, None]
    if where == "page_locked":
        outs = [engine.host_empty((N + 1) * 32).reshape(N + 1, 32) for _ in range(2)]
        assert all(o.ctypes.data % 16 == 0 for o in outs)
    ref = Run(engine, reqs, expected, outs[0])
    assert ref.mixed() == 0
    ref.wait()
    new = Run(engine, reqs, expected, outs[1])
    assert new.dedup() == 0
    assert int(new.unique[0]) == 9  # written before the call returns
    assert new.ticket.value == ref.ticket.value + 1
    new.wait()
    got = new.check(want)
    assert sorted(np.flatnonzero(got).tolist()) == sorted(wrong.values())
    ref.check(want)
    same_outputs(new, ref)
    # the rows the kernel gathered through are the host-only plan's
    row, unique = dedup_rows(reqs)
    assert unique == 9 and row.tolist() == [content_of(i) for i in range(N)]


def test_main_case_through_the_engine(engine, main_case):
    reqs, want, expected, wrong = main_case
    out = np.full((N, 32), 0xA5, dtype=np.uint8)
    t = engine.submit_slices_expect_dedup(reqs, expected, out=out)
    assert isinstance(t, ExpectTicket) and t.n_unique == 9 and t.mismatches is None
    assert engine.wait(t) is out
    assert t.mismatches.tolist() == sorted(wrong.values())  # the 20-byte expectation among them
    ref = engine.submit_slices_expect(reqs, expected, out=np.full((N, 32), 0xA5, dtype=np.uint8))
    assert np.array_equal(engine.wait(ref), out) and ref.mismatches.tolist() == t.mismatches.tolist()
    for i in range(N):
        kept = expected[i] is None or i in wrong.values()
        assert out[i].tobytes() == (want[i].tobytes() if kept else b"\xa5" * 32), i
    sync = engine.hash_slices_expect_dedup(reqs, expected, out=np.full((N, 32), 0xA5, dtype=np.uint8))
    assert sync.n_unique == 9 and sync.mismatches.tolist() == t.mismatches.tolist()
    assert np.array_equal(sync.out, out)


# ---- edge cases --------------------------------------------------------------------

def random_requests(seed, n, hi=200):
    rng = np.random.default_rng(seed)
    return [[rng.integers(0, 256, int(k), dtype=np.uint8).tobytes()] for k in rng.integers(0, hi + 1, n)]


def thirds(want, wrong=()):
    return [None if i % 3 else (wrong_row(want[i]) if i in wrong else want[i].tobytes())
            for i in range(want.shape[0])]


def run_and_check(engine, reqs, expected, unique):
    want = digests_of(reqs) if len(reqs) else np.zeros((0, 32), dtype=np.uint8)
    run = Run(engine, reqs, expected)
    assert run.dedup() == 0
    assert int(run.unique[0]) == unique and run.ticket.value > 0
    run.wait()
    return run, run.check(want)


def test_all_distinct(engine):
    reqs = [[bytes([i]) + r[0]] for i, r in enumerate(random_requests(1, 130))]
    want = digests_of(reqs)
    _, wrong = run_and_check(engine, reqs, thirds(want, {3, 66, 129}), 130)
    assert np.flatnonzero(wrong).tolist() == [3, 66, 129]


def test_all_identical(engine):
    reqs = [[b"epoch change ", b"payload" * 40] if i % 2 else [b"epoch change payload" + b"payload" * 39]
            for i in range(130)]  # every lane gathers row 0, whatever the slicing
    want = digests_of(reqs)
    _, wrong = run_and_check(engine, reqs, thirds(want, {0, 63, 66, 129}), 1)
    assert np.flatnonzero(wrong).tolist() == [0, 63, 66, 129]


def test_one_request_and_none(engine):
    for exp in (None, "right", "wrong"):
        reqs = [[b"only one"]]
        d = sha(reqs[0])
        run, wrong = run_and_check(engine, reqs, [None if exp is None else d if exp == "right" else bytes(32)], 1)
        assert wrong.tolist() == [exp == "wrong"]
    empty = SliceArrays(np.zeros(0, np.uint64), np.zeros(0, np.uint64), np.zeros(1, np.uint32))
    run = Run(engine, empty, [])
    assert run.dedup() == 0 and run.ticket.value > 0 and int(run.unique[0]) == 0
    run.wait()
    assert int(run.count[0]) == 0 and run.bits[0] == ONES and (run.out == 0xA5).all()


def test_no_expectation_writes_every_row(engine):
    reqs = [r for r in random_requests(2, 40) for _ in range(3)] + [[b"tail"]]
    _, wrong = run_and_check(engine, reqs, [None] * len(reqs), len({r[0] for r in reqs}))
    assert not wrong.any()


def test_every_expectation_matching_writes_no_row(engine):
    reqs = [r for r in random_requests(3, 26) for _ in range(5)]
    want = digests_of(reqs)
    run, wrong = run_and_check(engine, reqs, [w.tobytes() for w in want], len({r[0] for r in reqs}))
    assert not wrong.any() and (run.out == 0xA5).all() and not run.bits[:run.words].any()


# ---- the second launch -------------------------------------------------------------

def later_contents_case():
    """200 one-slice requests, so MIRSHA_DEDUP_SEGMENT_SLICES=40 makes five
    segments.  The first holds contents 0-5; contents 6-13 appear only in later
    segments (the second launch), where copies of all fourteen mix: duplicates
    point into both launches.  Lengths repeat, so with MIRSHA_DEDUP_WEAK_FP=1
    same-length contents collide and are settled byte for byte; the loser of
    such a collision is hashed in the second launch even when it lies in the
    first segment (contents 3 and 4)."""
    rng = np.random.default_rng(40)
    lens = [0, 1, 55, 64, 64, 119, 64, 55, 300, 300, 1, 56, 600, 119]
    pool = [(bytes([c]) + rng.integers(0, 256, k, dtype=np.uint8).tobytes())[:k] for c, k in enumerate(lens)]
    assert len(set(pool)) == 14
    which = [int(rng.integers(0, 6)) for _ in range(40)] + [int(rng.integers(0, 14)) for _ in range(160)]
    assert set(which[:40]) == set(range(6)) and set(which[40:]) == set(range(14))
    reqs = [[pool[c]] for c in which]
    want = digests_of(reqs)
    expected = thirds(want, {0, 42, 99, 150, 198})
    return reqs, want, expected


def child_second_launch():
    """Runs in a child process under the test knobs (read once per process)."""
    import torch

    torch.cuda.is_available()
    from mirbft_amd import Engine

    e = Engine(0)
    reqs, want, expected = later_contents_case()
    row, unique = dedup_rows(reqs)
    assert unique == 14
    m0 = len({len(r[0]) for r in reqs[:40]})  # weak fingerprints: one head per length in the first segment
    assert m0 == 5 and int(row[:40].max()) >= m0 and int(row.max()) == 13
    assert sorted(set(row.tolist())) == list(range(14))
    assert (row[40:] < m0).any() and (row[40:] >= m0).any()  # duplicates point into both launches
    ref = Run(e, reqs, expected)
    assert ref.mixed() == 0
    ref.wait().check(want)
    for where in ("pageable", "page_locked"):
        out = e.host_empty(201 * 32).reshape(201, 32) if where == "page_locked" else None
        run = Run(e, reqs, expected, out)
        assert run.dedup() == 0 and int(run.unique[0]) == 14
        wrong = run.wait().check(want)
        assert np.flatnonzero(wrong).tolist() == [0, 42, 99, 150, 198]
        same_outputs(run, ref)
    # a NULL slice with bytes in a later segment, after the first launch was queued
    last = run.ticket.value
    bad = Run(e, reqs, expected)
    at = next(i for i in range(150, 200) if reqs[i][0])
    bad.sl.ptr[at] = 0
    assert bad.dedup() == _lib.MIRSHA_EINVAL and bad.ticket.value == 0 and bad.untouched()
    assert b"request %d has a NULL slice" % at in e._lib.mirsha_last_error(e.ctx)
    nxt = Run(e, reqs, expected)
    assert nxt.dedup() == 0 and nxt.ticket.value == last + 1
    nxt.wait().check(want)
    e.close()
    print("ok")


def test_second_launch_in_a_child_process():
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import test_gpu_expect_dedup as t\n"
            "t.child_second_launch()\n" % (ROOT, os.path.join(ROOT, "tests")))
    env = dict(os.environ, MIRSHA_AB="1", MIRSHA_DEDUP_SEGMENT_SLICES="40", MIRSHA_DEDUP_WEAK_FP="1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=180)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-2000:]


# ---- refusals ----------------------------------------------------------------------

def test_refusals_queue_nothing_and_consume_no_ticket(engine, main_case):
    reqs, want, expected, _ = main_case
    good = Run(engine, reqs, expected)
    assert good.dedup() == 0
    good.wait().check(want)
    last = good.ticket.value
    rows = np.ascontiguousarray(want[:2])

    def refused(**how):
        nonlocal last
        run = Run(engine, reqs, expected)
        null_slice = how.pop("null_slice", None)
        if null_slice is not None:
            run.sl.ptr[int(run.sl.first[null_slice])] = 0
        assert run.dedup(**how) == _lib.MIRSHA_EINVAL
        assert run.ticket.value == 0 and run.untouched()
        assert engine._lib.mirsha_last_error(engine.ctx)
        nxt = Run(engine, reqs, expected)  # the next submission takes the next ticket and is correct
        assert nxt.dedup() == 0 and nxt.ticket.value == last + 1
        last += 1
        nxt.wait().check(want)

    refused(of=[5, 3], rows_p=rows.ctypes.data)              # not increasing
    refused(of=[3, 3], rows_p=rows.ctypes.data)              # a duplicate index
    refused(of=[3, N], rows_p=rows.ctypes.data)              # an index >= n
    refused(of=[3, 4], rows_p=None)                          # NULL expected with m > 0
    refused(of=[3, 4], rows_p=rows.ctypes.data, count_p=None)  # NULL n_mismatch_out
    refused(null_slice=120)                                  # a NULL slice with bytes, late in the cycle
    assert reqs[120][0]  # (its first slice has bytes)


# ---- the ring ----------------------------------------------------------------------

def test_ring_six_tickets_waited_out_of_order(engine, main_case):
    reqs, want, expected, wrong = main_case
    rng = np.random.default_rng(6)
    filled = lambda: np.full((N, 32), 0xA5, dtype=np.uint8)
    ch = CheckpointChains(engine, 3)
    table = rng.integers(0, 256, (8, 32), dtype=np.uint8)
    cp = _lib.MIRSHA_COMMIT_CHECKPOINT
    other = random_requests(60, 70)
    t = [engine.submit_slices_expect_dedup(reqs, expected, out=filled()),  # the new form
         engine.submit_slices(other),                                       # plain
         engine.submit_slices(reqs, dedup=True),                            # DEDUP
         engine.submit_slices_expect(reqs, expected, out=filled()),         # mixed
         ch.submit_commit(table, [0, 1, 0, 0], [2, 5, 7, cp]),              # a commit ticket
         engine.submit_slices_expect_dedup(list(reversed(reqs)), list(reversed(expected)), out=filled())]
    assert [x.value for x in t] == list(range(t[0].value, t[0].value + 6))
    kept = np.asarray([e is None or i in wrong.values() for i, e in enumerate(expected)])
    masked = np.where(kept[:, None], want, np.uint8(0xA5))

    def check(k):
        if k in (0, 3):
            assert np.array_equal(t[k].out, masked) and t[k].mismatches.tolist() == sorted(wrong.values())
        elif k == 1:
            assert np.array_equal(t[k].out, digests_of(other))
        elif k == 2:
            assert np.array_equal(t[k].out, want)
        elif k == 4:
            assert [v.tobytes() for v in t[k].values] == [
                hashlib.sha256(table[2].tobytes() + table[7].tobytes()).digest()]
        else:
            assert np.array_equal(t[k].out, masked[::-1])
            assert t[k].mismatches.tolist() == sorted(N - 1 - i for i in wrong.values()) and t[k].n_unique == 9

    engine.wait(t[2])  # retires tickets 0-2
    for k in (2, 0, 1):
        if isinstance(t[k], ExpectTicket):
            t[k]._resolve()
        check(k)
    while not engine.poll(t[4]):  # the one poll: retires 3 and 4 when it reports done
        pass
    engine.wait(t[5])
    engine.wait(t[3])  # already retired: resolves its verdict
    for k in (5, 4, 3):
        check(k)
    ch.close()


# ---- Processor ---------------------------------------------------------------------

def test_processor_submit_is_one_ticket(engine):
    rng = np.random.default_rng(21)
    distinct = []
    for i in range(60):  # 1-3 slices, 0..600 bytes (content 17 is empty)
        total = 0 if i == 17 else int(rng.integers(0, 601))
        cuts = sorted(int(c) for c in rng.integers(0, total + 1, int(rng.integers(0, 3))))
        blob = rng.integers(0, 256, total, dtype=np.uint8).tobytes()
        distinct.append([blob[a:b] for a, b in zip([0] + cuts, cuts + [total])])
    reqs = [distinct[int(c)] for c in rng.integers(0, 60, 300)]
    want = digests_of(reqs)
    wrong = {3, 150, 297, 33}
    cycle = []
    for i, data in enumerate(reqs):
        exp = None
        if i % 3 == 0:
            exp = want[i].tobytes()
            if i in wrong:
                exp = bytes(32) if i != 33 else exp[:20]  # 33: an expectation of the wrong length
        cycle.append(HashRequest(data, ("origin", i), exp))
    plain = Processor(engine).process(Actions(hash=cycle))
    assert [r.digest for r in plain.digests] == [want[i].tobytes() for i in range(300)]
    before = engine.submit_slices([[b"ticket counter"]])
    engine.wait(before)
    got = Processor(engine, dedup=True, verify_on_device=True).submit(Actions(hash=cycle)).wait()
    after = engine.submit_slices([[b"ticket counter"]])
    engine.wait(after)
    assert after.value == before.value + 2  # the cycle took exactly one ticket
    assert [r.digest for r in got.digests] == [r.digest for r in plain.digests]
    assert all(a.request is b for a, b in zip(got.digests, cycle))
    assert got.checkpoints == []
