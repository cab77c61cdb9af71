"""A ring slot retired as one kind of ticket and reused as another carries
nothing over.  For every ordered pair (A, B) of the seven ticket kinds: submit
A, three one-request fillers (the ring has four slots), then B, which lands on
A's slot; then wait for everything and check A's and B's results, every byte,
against hashlib: digests, kept rows and the guard in the rows that must stay
untouched, mismatch bitmap and count, checkpoint values, n_unique.

The cycle is the smallest that takes every retirement route: 130 requests (two
full bitmap words and a partial one) of 0 to 120 bytes (one to three blocks, so
the bucket order is no identity), about a third of them copies of earlier ones
(the dedup fan-out is no identity), an expectation on every third request, two
of them wrong, one of those on a copy; the commit programme has 3 chains, 9 ops
and 2 checkpoints over 8 digests."""
import hashlib

import numpy as np
import pytest

from mirbft_amd import CheckpointChains, _lib
from mirbft_amd.engine import ASYNC_SLOTS

pytestmark = pytest.mark.gpu

N = 130
LENGTHS = (0, 1, 55, 56, 64, 119, 120)
GUARD = 0xA5
CP = _lib.MIRSHA_COMMIT_CHECKPOINT
KINDS = ["slices", "slices_dedup", "batch_pageable", "batch_host", "expect", "expect_dedup", "commit"]
KERNEL_WRITABLE = {"expect", "expect_dedup", "commit"}  # kinds whose kernel stores into a page-locked `out` itself


def sha(*parts):
    return hashlib.sha256(b"".join(parts)).digest()


class Case:
    pass


@pytest.fixture(scope="module")
def case():
    """The cycle and everything hashlib says about it, computed once."""
    rng = np.random.default_rng(130)
    c = Case()
    content, copy = [], []
    for i in range(N):
        if i and rng.random() < 1 / 3:
            content.append(content[int(rng.integers(0, i))])
        else:
            k = int(rng.choice(LENGTHS))
            content.append(rng.integers(0, 256, k, dtype=np.uint8).tobytes())
        copy.append(content[i] in content[:i])
    assert 30 <= sum(copy) <= 60
    c.unique = len(set(content))
    assert c.unique == N - sum(copy)
    blocks = [(len(b) + 72) >> 6 for b in content]
    assert set(blocks) == {1, 2, 3} and blocks != sorted(blocks, reverse=True)
    # two slices where there is something to cut
    c.reqs = [[b[:len(b) // 2], b[len(b) // 2:]] if len(b) > 1 and i % 2 else [b] for i, b in enumerate(content)]
    c.ln = np.asarray([len(b) for b in content], dtype=np.uint32)
    c.off = np.zeros(N, dtype=np.uint64)
    np.cumsum(c.ln[:-1].astype(np.uint64), out=c.off[1:])
    c.arena = np.frombuffer(b"".join(content) + b"\0", dtype=np.uint8)
    c.want = np.frombuffer(b"".join(sha(b) for b in content), dtype=np.uint8).reshape(N, 32)
    c.want.setflags(write=False)
    # an expectation on every third request; a first occurrence and a copy are wrong, in different words
    holders = list(range(0, N, 3))
    c.wrong = sorted([next(i for i in holders if not copy[i] and i < 64), next(i for i in holders if copy[i] and i >= 64)])
    c.expected = [None] * N
    for i in holders:
        row = bytearray(c.want[i].tobytes())
        if i in c.wrong:
            row[i % 32] ^= 0x40
        c.expected[i] = bytes(row)
    kept = np.ones(N, dtype=bool)
    kept[holders] = False
    kept[c.wrong] = True
    c.masked = np.where(kept[:, None], c.want, np.uint8(GUARD))
    flags = np.zeros(192, dtype=np.uint8)
    flags[c.wrong] = 1
    c.bits = np.packbits(flags, bitorder="little").view(np.uint64)
    # the commit programme: chain 1's checkpoint after one write, chain 0's after three
    c.table = rng.integers(0, 256, (8, 32), dtype=np.uint8)
    c.op_chain = [0, 1, 0, 2, 1, 0, 2, 1, 0]
    c.op_digest = [0, 1, 2, 3, CP, 4, 5, 7, CP]
    t = [row.tobytes() for row in c.table]
    c.values = [sha(t[1]), sha(t[0], t[2], t[4])]
    c.sums = [sha(), sha(t[7]), sha(t[3], t[5])]
    return c


class Submission:
    """One ticket of `kind`; ``pinned``: its result rows are page-locked."""

    def __init__(self, engine, c, kind, pinned=False):
        self.engine, self.c, self.kind = engine, c, kind
        rows = 2 if kind == "commit" else N
        if pinned or kind == "batch_host":
            self.out = engine.host_empty(32 * rows).reshape(rows, 32)
            assert self.out.ctypes.data % 16 == 0
        else:
            self.out = np.empty((rows, 32), dtype=np.uint8)
        self.out[:] = GUARD
        self.chains = None
        if kind == "slices":
            self.ticket = engine.submit_slices(c.reqs)
        elif kind == "slices_dedup":
            self.ticket = engine.submit_slices(c.reqs, dedup=True)
        elif kind in ("batch_pageable", "batch_host"):
            self.ticket = engine.submit_batch(c.arena, c.off, c.ln, out=self.out)
        elif kind == "expect":
            self.ticket = engine.submit_slices_expect(c.reqs, c.expected, out=self.out)
        elif kind == "expect_dedup":
            self.ticket = engine.submit_slices_expect_dedup(c.reqs, c.expected, out=self.out)
        else:
            self.chains = CheckpointChains(engine, 3)
            self.ticket = self.chains.submit_commit(c.table, c.op_chain, c.op_digest, out=self.out)

    def check(self, what):
        c, t = self.c, self.ticket
        out = self.engine.wait(t)  # retired already: resolves the verdict
        if self.kind in ("slices", "slices_dedup"):
            assert np.array_equal(out, c.want), what
        elif self.kind in ("batch_pageable", "batch_host"):
            assert out is self.out and np.array_equal(out, c.want), what
        elif self.kind in ("expect", "expect_dedup"):
            assert out is self.out
            assert np.array_equal(out, c.masked), what  # kept rows are hashlib's, the others still hold the guard
            assert np.array_equal(t._bits, c.bits) and int(t._count[0]) == len(c.wrong), what
            assert t.mismatches.tolist() == c.wrong, what
            assert t.n_unique == (c.unique if self.kind == "expect_dedup" else None), what
        else:
            assert out is self.out and [v.tobytes() for v in out] == c.values, what
            assert [s.tobytes() for s in self.chains.sum(np.arange(3, dtype=np.uint32))] == c.sums, what
            self.chains.close()


@pytest.mark.parametrize("b_rows", ["pageable", "page_locked"])
@pytest.mark.parametrize("a_rows", ["pageable", "page_locked"])
def test_every_pair_of_kinds_on_one_slot(engine, case, a_rows, b_rows):
    """``page_locked``: the pairs whose A (B) has a kernel-writable route, with
    those rows page-locked, so the slot goes from "the kernel wrote the caller's
    rows" to "copy at retirement" and back."""
    ran = 0
    for a_kind in KINDS:
        if a_rows == "page_locked" and a_kind not in KERNEL_WRITABLE:
            continue
        for b_kind in KINDS:
            if b_rows == "page_locked" and b_kind not in KERNEL_WRITABLE:
                continue
            what = f"{a_kind} ({a_rows}) then {b_kind} ({b_rows})"
            a = Submission(engine, case, a_kind, a_rows == "page_locked")
            fillers = [(engine.submit_slices([[b"filler %d" % k]]), sha(b"filler %d" % k))
                       for k in range(ASYNC_SLOTS - 1)]
            b = Submission(engine, case, b_kind, b_rows == "page_locked")
            assert b.ticket.value == a.ticket.value + ASYNC_SLOTS, what  # A's slot
            engine.wait(b.ticket)  # retires everything before it, in order
            a.check(what + ": A")
            for t, want in fillers:
                assert engine.wait(t).tobytes() == want, what
            b.check(what + ": B")
            ran += 1
    n_a = len(KERNEL_WRITABLE) if a_rows == "page_locked" else len(KINDS)
    n_b = len(KERNEL_WRITABLE) if b_rows == "page_locked" else len(KINDS)
    assert ran == n_a * n_b
