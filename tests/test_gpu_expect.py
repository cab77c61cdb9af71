"""Mixed hash-and-verify cycles in the asynchronous ring
(mirsha_submit_slices_expect / mirsha_submit_batch_expect /
mirsha_hash_slices_expect, expect_select_kernel): each request may or may not
carry the digest its origin expects; the verdict, and the digests of the
requests without an expectation and of the mismatches, come back -- the rows
of matching requests are never written.  Everything is compared with hashlib.

Every output is pre-filled: digests_out with 0xA5 plus one guard row, the
bitmap with 0xFF plus one guard word, the count with 0xDEADBEEF."""
import ctypes
import hashlib

import numpy as np
import pytest

from mirbft_amd import (Actions, ExpectTicket, HashRequest, Processor, ProcessorWorkPool, SliceArrays, _lib,
                        expect_plan, mismatch_indices)

pytestmark = pytest.mark.gpu

BLOCK = 256  # expect_select_kernel: one request per lane, 256-thread workgroups, no grid-stride loop
ONES = np.uint64(0xFFFFFFFFFFFFFFFF)


def _p(a):
    return a.ctypes.data if a is not None and a.size else None


def messages(seed, n, hi=200):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, int(k), dtype=np.uint8).tobytes() for k in rng.integers(0, hi + 1, n)]


def digests_of(msgs):
    return np.frombuffer(b"".join(hashlib.sha256(m).digest() for m in msgs), dtype=np.uint8).reshape(len(msgs), 32)


def random_expectations(seed, want, p_has=0.5, p_wrong=0.10):
    """One Optional[bytes] per request: an expectation with probability p_has,
    about p_wrong of those wrong in one random byte."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(want.shape[0]):
        if rng.random() >= p_has:
            out.append(None)
            continue
        row = want[i].copy()
        if rng.random() < p_wrong:
            row[int(rng.integers(0, 32))] ^= np.uint8(rng.integers(1, 256))
        out.append(row.tobytes())
    return out


def packed(msgs, gap=0):
    """(arena, off, len): the messages back to back, `gap` bytes apart."""
    ln = np.asarray([len(m) for m in msgs], dtype=np.uint32)
    off = np.zeros(len(msgs), dtype=np.uint64)
    if len(msgs) > 1:
        off[1:] = np.cumsum(ln[:-1].astype(np.uint64) + np.uint64(gap))
    arena = np.full(int(off[-1]) + int(ln[-1]) + gap if len(msgs) else 0, 0xEE, dtype=np.uint8)
    for m, o in zip(msgs, off):
        arena[int(o):int(o) + len(m)] = np.frombuffer(m, dtype=np.uint8)
    return arena, off, ln


class Run:
    """One raw mirsha_submit_*_expect call with pre-filled outputs; keeps every
    array the library reads or writes alive."""

    def __init__(self, engine, n, expected, out=None):
        self.engine, self.n, self.expected = engine, n, list(expected)
        self.of, self.rows, self.short = expect_plan(self.expected)
        assert self.short.size == 0
        self.words = (n + 63) // 64
        self.out = np.empty((n + 1, 32), dtype=np.uint8) if out is None else out
        assert self.out.shape == (n + 1, 32)
        self.out[:] = 0xA5
        self.bits = np.full(self.words + 1, ONES, dtype=np.uint64)
        self.count = np.full(1, 0xDEADBEEF, dtype=np.uint32)
        self.ticket = ctypes.c_uint64(0)
        self.keep = None

    def slices(self, msgs, flags=0):
        sl = msgs if isinstance(msgs, SliceArrays) else SliceArrays.from_requests([[m] for m in msgs])
        self.keep = sl
        return self.engine._lib.mirsha_submit_slices_expect(
            self.engine.ctx, sl.ptr_p, sl.len_p, sl.first_p, sl.n, _p(self.of), _p(self.rows), self.of.size,
            self.out.ctypes.data, self.bits.ctypes.data, self.count.ctypes.data, flags, ctypes.byref(self.ticket))

    def batch(self, arena, off, ln):
        self.keep = (arena, off, ln)
        return self.engine._lib.mirsha_submit_batch_expect(
            self.engine.ctx, _p(arena), arena.size, _p(off), _p(ln), off.size, _p(self.of), _p(self.rows),
            self.of.size, self.out.ctypes.data, self.bits.ctypes.data, self.count.ctypes.data,
            ctypes.byref(self.ticket))

    def wait(self):
        assert self.engine._lib.mirsha_wait(self.engine.ctx, self.ticket.value) == 0
        return self

    def untouched(self):
        return int(self.count[0]) == 0xDEADBEEF and bool((self.out == 0xA5).all()) and bool((self.bits == ONES).all())

    def check(self, want):
        """The whole contract of a retired ticket against the hashlib digests."""
        n = self.n
        has = np.asarray([e is not None for e in self.expected], dtype=bool)
        wrong = np.zeros(n, dtype=bool)
        for i in np.flatnonzero(has):
            wrong[i] = self.expected[i] != want[i].tobytes()
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


# ---- sizes ----------------------------------------------------------------------
# One n past everything a single wave, a single workgroup and a power of two
# cover; the kernel has no grid-stride loop, so the largest size only has to
# span many workgroups and end inside a wave.
@pytest.mark.parametrize("n", [1, 63, 64, 65, 127, 128, 129, 1000, 40 * BLOCK + 37])
def test_sizes(engine, n):
    msgs = messages(n, n)
    want = digests_of(msgs)
    expected = random_expectations(n + 1, want)
    run = Run(engine, n, expected)
    assert run.slices(msgs) == 0
    wrong = run.wait().check(want)
    if n >= 1000:
        assert wrong.any() and not wrong.all()
    # the arena form over the same cycle
    run = Run(engine, n, expected)
    assert run.batch(*packed(msgs)) == 0
    run.wait().check(want)


# ---- masks at n = 130 -------------------------------------------------------------

@pytest.fixture(scope="module")
def case130():
    msgs = messages(130, 130)
    return msgs, digests_of(msgs)


def wrong_row(row):
    bad = row.copy()
    bad[31] ^= 0x01
    return bad.tobytes()


def test_no_expectation_equals_submit_slices(engine, case130):
    msgs, want = case130
    run = Run(engine, 130, [None] * 130)
    assert run.slices(msgs) == 0
    run.wait().check(want)
    assert np.array_equal(run.out[:130], engine.wait(engine.submit_slices([[m] for m in msgs])))
    assert int(run.count[0]) == 0 and not run.bits[:3].any()


def test_all_expected_all_match_writes_no_row(engine, case130):
    msgs, want = case130
    run = Run(engine, 130, [want[i].tobytes() for i in range(130)])
    assert run.slices(msgs) == 0
    run.wait().check(want)
    assert int(run.count[0]) == 0 and (run.out == 0xA5).all()


def test_all_expected_all_wrong(engine, case130):
    msgs, want = case130
    run = Run(engine, 130, [wrong_row(want[i]) for i in range(130)])
    assert run.slices(msgs) == 0
    run.wait().check(want)
    assert int(run.count[0]) == 130 and np.array_equal(run.out[:130], want)


@pytest.mark.parametrize("at", [0, 129, 63, 64])
@pytest.mark.parametrize("matching", [True, False])
def test_single_expectation(engine, case130, at, matching):
    msgs, want = case130
    expected = [None] * 130
    expected[at] = want[at].tobytes() if matching else wrong_row(want[at])
    run = Run(engine, 130, expected)
    assert run.slices(msgs) == 0
    run.wait().check(want)
    assert mismatch_indices(run.bits, 130).tolist() == ([] if matching else [at])
    assert (run.out[at] == 0xA5).all() == matching


# ---- every bit counts -------------------------------------------------------------

def test_every_bit_of_the_digest_counts(engine):
    msgs = messages(256, 257)
    want = digests_of(msgs)
    expected = []
    for r in range(256):
        row = want[r].copy()
        row[r >> 3] ^= np.uint8(1 << (r & 7))
        expected.append(row.tobytes())
    expected.append(want[256].tobytes())  # the exact control
    run = Run(engine, 257, expected)
    assert run.slices(msgs) == 0
    wrong = run.wait().check(want)
    assert wrong[:256].all() and not wrong[256] and int(run.count[0]) == 256


# ---- origin order under a permuted processing order ---------------------------------

def test_origin_order_with_mixed_block_counts(engine):
    rng = np.random.default_rng(77)
    lengths = rng.permutation(601)  # 0..600 bytes, 1..10 blocks: the bucket order is not the identity
    msgs = [rng.integers(0, 256, int(k), dtype=np.uint8).tobytes() for k in lengths]
    want = digests_of(msgs)
    bad = [0, 5, 63, 64, 300, 599, 600]
    expected = [want[i].tobytes() if i % 2 == 0 or i in bad else None for i in range(601)]
    for i in bad:
        expected[i] = wrong_row(want[i])
    for form in ("slices", "batch"):
        run = Run(engine, 601, expected)
        assert (run.slices(msgs) if form == "slices" else run.batch(*packed(msgs))) == 0
        run.wait().check(want)
        assert mismatch_indices(run.bits, 601).tolist() == bad
        assert np.array_equal(run.out[bad], want[bad])


# ---- arena form -------------------------------------------------------------------

def pinned_rows(engine, n, shift=0):
    """(n + 1, 32) rows in page-locked memory, `shift` bytes past the allocation's start."""
    buf = engine.host_empty(32 * (n + 1) + 16)
    return buf[shift:shift + 32 * (n + 1)].reshape(n + 1, 32)


@pytest.fixture(scope="module")
def case700():
    msgs = messages(700, 700)
    want = digests_of(msgs)
    return msgs, want, random_expectations(701, want)


# gapless and with gaps (a dense arena: DMA'd or copied as one span), and a
# sparse one (span > 2 * total + 4096: packed back to back into the staging)
@pytest.mark.parametrize("arena_kind,gap", [("pageable", 0), ("pageable", 5), ("pinned", 0), ("pinned", 5),
                                            ("sparse", 4096)])
@pytest.mark.parametrize("out_kind", ["pageable", "pinned", "pinned+8"])
def test_arena_routes(engine, case700, arena_kind, gap, out_kind):
    msgs, want, expected = case700
    arena, off, ln = packed(msgs, gap)
    assert (int((off + ln).max() - off.min()) > 2 * int(ln.sum()) + 4096) == (arena_kind == "sparse")
    if arena_kind == "pinned":
        held = engine.host_empty(arena.size)
        held[:] = arena
        arena = held
    out = None if out_kind == "pageable" else pinned_rows(engine, 700, 8 if out_kind == "pinned+8" else 0)
    if out is not None:
        assert (out.ctypes.data & 15) == (8 if out_kind == "pinned+8" else 0)
    run = Run(engine, 700, expected, out)
    assert run.batch(arena, off, ln) == 0
    wrong = run.wait().check(want)
    assert wrong.any()


def test_engine_api_and_synchronous_form(engine, case700):
    msgs, want, expected = case700
    expected = list(expected)
    first = next(i for i, e in enumerate(expected) if e is not None)
    expected[first] = expected[first][:20]  # the wrong length: a mismatch already on the host
    has = np.asarray([e is not None for e in expected])
    wrong = [i for i in np.flatnonzero(has) if expected[i] != want[i].tobytes()]
    out = np.full((700, 32), 0xA5, dtype=np.uint8)
    t = engine.submit_slices_expect([[m] for m in msgs], expected, out=out)
    assert isinstance(t, ExpectTicket) and t.mismatches is None and np.array_equal(t.has, has)
    assert engine.wait(t) is out and t.mismatches.tolist() == wrong
    keep = ~has
    keep[wrong] = True
    assert np.array_equal(out[keep], want[keep]) and (out[~keep] == 0xA5).all()
    t = engine.submit_batch_expect(*packed(msgs), expected)
    while not engine.poll(t):
        pass
    assert t.mismatches.tolist() == wrong and np.array_equal(t.out[keep], want[keep])
    # mirsha_hash_slices_expect: submit + wait
    run = Run(engine, 700, case700[2])
    sl = SliceArrays.from_requests([[m] for m in msgs])
    rc = engine._lib.mirsha_hash_slices_expect(engine.ctx, sl.ptr_p, sl.len_p, sl.first_p, 700, _p(run.of),
                                               _p(run.rows), run.of.size, run.out.ctypes.data, run.bits.ctypes.data,
                                               run.count.ctypes.data)
    assert rc == 0
    run.check(want)
    prof = engine.host_profile()
    assert prof["device"] > 0 and prof["scatter"] >= 0 and prof["pack"] > 0


# ---- ring -------------------------------------------------------------------------

def test_ring_of_mixed_and_plain_submissions(engine):
    cases = []
    for k in range(6):
        msgs = messages(900 + k, 200 + 17 * k)
        want = digests_of(msgs)
        cases.append((msgs, want, random_expectations(950 + k, want)))
    runs = []
    for k, (msgs, want, expected) in enumerate(cases):
        if k % 3 == 2:
            runs.append(engine.submit_slices([[m] for m in msgs]))
        else:
            run = Run(engine, len(msgs), expected)
            assert (run.slices(msgs) if k % 3 == 0 else run.batch(*packed(msgs))) == 0
            runs.append(run)
        if k == 4:  # the fifth submission took the first's slot: the first is complete now
            runs[0].check(cases[0][1])
    values = [r.ticket.value if isinstance(r, Run) else r.value for r in runs]
    assert values == list(range(values[0], values[0] + 6))
    engine.wait(runs[5])  # the last: everything before it is complete too
    for k, r in enumerate(runs):
        if isinstance(r, Run):
            r.check(cases[k][1])
        else:
            assert np.array_equal(r.out, cases[k][1])


def test_wait_completes_earlier_tickets_and_poll(engine):
    msgs = messages(31, 300)
    want = digests_of(msgs)
    expected = random_expectations(32, want)
    runs = [Run(engine, 300, expected) for _ in range(4)]
    for k, run in enumerate(runs):
        assert (run.batch(*packed(msgs)) if k % 2 else run.slices(msgs)) == 0
    assert engine._lib.mirsha_wait(engine.ctx, runs[2].ticket.value) == 0
    for run in runs[:3]:  # wait(t3) completed tickets 1 to 3
        run.check(want)
    done = ctypes.c_int(0)
    while not done.value:  # poll until done: writes the outputs when it reports done
        assert engine._lib.mirsha_poll(engine.ctx, runs[3].ticket.value, ctypes.byref(done)) == 0
        if not done.value:
            assert runs[3].untouched()
    runs[3].check(want)


# ---- errors -----------------------------------------------------------------------

def test_invalid_arguments_queue_nothing(engine, case130):
    msgs, want = case130
    lib, ctx = engine._lib, engine.ctx
    sl = SliceArrays.from_requests([[m] for m in msgs])
    arena, off, ln = packed(msgs)
    good = Run(engine, 130, [want[0].tobytes()] + [None] * 129)
    assert good.slices(msgs) == 0
    good.wait().check(want)
    last = good.ticket.value
    rows = np.ascontiguousarray(want[:2])

    def attempt(of, rows_p, m, count_p, flags=0, form="slices"):
        nonlocal last
        out = np.full((131, 32), 0xA5, dtype=np.uint8)
        bits = np.full(4, ONES, dtype=np.uint64)
        t = ctypes.c_uint64(0)
        of = np.asarray(of, dtype=np.uint32)
        if form == "slices":
            rc = lib.mirsha_submit_slices_expect(ctx, sl.ptr_p, sl.len_p, sl.first_p, 130, _p(of), rows_p, m,
                                                 out.ctypes.data, bits.ctypes.data, count_p, flags, ctypes.byref(t))
        else:
            rc = lib.mirsha_submit_batch_expect(ctx, _p(arena), arena.size, _p(off), _p(ln), 130, _p(of), rows_p, m,
                                                out.ctypes.data, bits.ctypes.data, count_p, ctypes.byref(t))
        assert rc == _lib.MIRSHA_EINVAL and t.value == 0
        assert lib.mirsha_last_error(ctx)
        assert (out == 0xA5).all() and (bits == ONES).all()
        # no ticket was consumed and the context stays usable
        nxt = Run(engine, 130, [None, wrong_row(want[1])] + [None] * 128)
        assert (nxt.slices(msgs) if form == "slices" else nxt.batch(arena, off, ln)) == 0
        assert nxt.ticket.value == last + 1
        last += 1
        nxt.wait().check(want)

    count = np.full(1, 0xDEADBEEF, dtype=np.uint32)
    for form in ("slices", "batch"):
        attempt([5, 3], rows.ctypes.data, 2, count.ctypes.data, form=form)       # not increasing
        attempt([3, 3], rows.ctypes.data, 2, count.ctypes.data, form=form)       # a duplicate
        attempt([3, 130], rows.ctypes.data, 2, count.ctypes.data, form=form)     # an index >= n
        attempt([3, 4], None, 2, count.ctypes.data, form=form)                   # NULL expected with m > 0
        attempt([3, 4], rows.ctypes.data, 2, None, form=form)                    # NULL n_mismatch_out
    attempt([3, 4], rows.ctypes.data, 2, count.ctypes.data, flags=_lib.MIRSHA_SUBMIT_DEDUP)
    attempt([3, 4], rows.ctypes.data, 2, count.ctypes.data, flags=2)
    assert int(count[0]) == 0xDEADBEEF


def test_empty_submission(engine):
    for form in ("slices", "batch"):
        run = Run(engine, 0, [])
        if form == "slices":
            assert run.slices(SliceArrays(np.zeros(0, np.uint64), np.zeros(0, np.uint64), np.zeros(1, np.uint32))) == 0
        else:
            assert run.batch(np.zeros(0, np.uint8), np.zeros(0, np.uint64), np.zeros(0, np.uint32)) == 0
        assert run.ticket.value > 0
        run.wait()
        assert int(run.count[0]) == 0 and run.bits[0] == ONES and (run.out == 0xA5).all()


# ---- Processor ----------------------------------------------------------------------

def test_processor_submit_and_pool_equal_plain(engine):
    rng = np.random.default_rng(21)
    reqs = []
    for i in range(300):  # 1-3 slices, 0..600 bytes (request 17 is empty)
        total = 0 if i == 17 else int(rng.integers(0, 601))
        cuts = sorted(int(c) for c in rng.integers(0, total + 1, int(rng.integers(0, 3))))
        blob = rng.integers(0, 256, total, dtype=np.uint8).tobytes()
        reqs.append([blob[a:b] for a, b in zip([0] + cuts, cuts + [total])])
    want = digests_of([b"".join(r) for r in reqs])
    wrong = {3, 150, 297, 33}
    cycle = []
    for i, data in enumerate(reqs):
        exp = None
        if i % 3 == 0:
            exp = want[i].tobytes()
            if i in wrong:
                exp = bytes(32) if i != 33 else exp[:20]  # 33: an expectation of the wrong length
        cycle.append(HashRequest(data, ("origin", i), exp))
    assert sum(r.expected is not None for r in cycle) == 100
    plain = Processor(engine).process(Actions(hash=cycle))
    assert [r.digest for r in plain.digests] == [want[i].tobytes() for i in range(300)]
    ran = []
    for got in (Processor(engine, verify_on_device=True).submit(Actions(hash=cycle)).wait(),
                ProcessorWorkPool(engine, verify_on_device=True).process(Actions(hash=cycle),
                                                                         overlap=lambda: ran.append(1)),
                ProcessorWorkPool(engine, dedup=True, verify_on_device=True).process(Actions(hash=cycle))):
        assert [r.digest for r in got.digests] == [r.digest for r in plain.digests]
        assert all(a.request is b for a, b in zip(got.digests, cycle))
        assert got.checkpoints == []
    assert ran == [1]
