"""Host side of the deduplicated mixed ring submission (no GPU):
Processor.submit / ProcessorWorkPool.process with ``dedup=True,
verify_on_device=True`` over the hashlib stand-in ring of
tests/test_expect_host.py, with and without ``submit_slices_expect_dedup``;
and mirsha_dedup_rows -- the rows the call sends its select kernel -- through
ctypes against a Python restatement, also under the segment and
weak-fingerprint test knobs (read once per process, hence child processes)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from mirbft_amd import Actions, HashRequest, Processor, ProcessorWorkPool, SliceArrays, _lib, dedup_plan, dedup_rows
from test_expect_host import HashlibRing, assert_same, mixed_cycle
from test_host_dedup import random_requests

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class DedupRing(HashlibRing):
    """The stand-in ring with the one-ticket call as well."""

    def submit_slices_expect_dedup(self, requests, expected):
        ticket = HashlibRing.submit_slices_expect(self, requests, expected)
        self.log[-1] = ("submit_slices_expect_dedup",) + self.log[-1][1:]
        ticket.n_unique = len({b"".join(bytes(s) for s in r) for r in requests})
        return ticket


def duplicated_cycle():
    """mixed_cycle with every request a second time: with its expectation, with
    a wrong one, and without one, in turn."""
    cycle = mixed_cycle()
    more = []
    for i, r in enumerate(cycle):
        exp = (r.expected, bytes(range(32)), None)[i % 3]
        more.append(HashRequest(r.data, ("copy", i), exp))
    return cycle + more


# ---- Processor over the stand-in rings ------------------------------------------

@pytest.mark.parametrize("make", [mixed_cycle, duplicated_cycle])
def test_submit_is_one_submission_and_one_wait(make):
    cycle = make()
    n, m = len(cycle), sum(r.expected is not None for r in cycle)
    ring = DedupRing()
    pending = Processor(ring, dedup=True, verify_on_device=True).submit(Actions(hash=cycle))
    assert ring.log == [("submit_slices_expect_dedup", n, m)]
    got = pending.wait()
    assert_same(got, cycle)  # hashlib's digests, wrong-length expectations included; back-pointers
    assert ring.log == [("submit_slices_expect_dedup", n, m), ("wait", 1)]
    assert pending.wait() is got and len(ring.log) == 2
    plain = Processor(HashlibRing()).submit(Actions(hash=cycle)).wait()
    assert [r.digest for r in got.digests] == [r.digest for r in plain.digests]


def test_pool_submits_overlaps_then_waits():
    cycle = mixed_cycle()
    ring = DedupRing()
    pool = ProcessorWorkPool(ring, dedup=True, verify_on_device=True)
    got = pool.process(Actions(hash=cycle), overlap=lambda: ring.log.append(("overlap",)))
    assert_same(got, cycle)
    assert ring.log == [("submit_slices_expect_dedup", 90, 30), ("overlap",), ("wait", 1)]


def test_an_engine_without_the_call_gets_two_submissions():
    cycle = mixed_cycle()
    ring = HashlibRing()
    assert not hasattr(ring, "submit_slices_expect_dedup")
    pool = ProcessorWorkPool(ring, dedup=True, verify_on_device=True)
    got = pool.process(Actions(hash=cycle), overlap=lambda: ring.log.append(("overlap",)))
    assert_same(got, cycle)
    assert ring.log == [("submit_slices_expect", 30, 30), ("submit_slices", 60, True), ("overlap",), ("wait", 1),
                        ("wait", 2)]


def test_a_cycle_without_expectations_is_one_dedup_submission():
    none = [HashRequest(r.data, r.origin) for r in mixed_cycle()]
    ring = DedupRing()
    assert_same(Processor(ring, dedup=True, verify_on_device=True).submit(Actions(hash=none)).wait(), none)
    assert ring.log == [("submit_slices", 90, True), ("wait", 1)]
    # the flags one at a time keep their routes
    ring = DedupRing()
    cycle = mixed_cycle()
    assert_same(Processor(ring, verify_on_device=True).submit(Actions(hash=cycle)).wait(), cycle)
    assert [e[0] for e in ring.log] == ["submit_slices_expect", "wait"]
    ring = DedupRing()
    assert_same(Processor(ring, dedup=True).submit(Actions(hash=cycle)).wait(), cycle)
    assert ring.log == [("submit_slices", 90, True), ("wait", 1)]
    ring = DedupRing()
    assert_same(Processor(ring, dedup=True, verify_on_device=True).process(Actions(hash=cycle)), cycle)
    assert [e[0] for e in ring.log] == ["verify_slices", "hash_slices"]  # process(): the synchronous split


# ---- mirsha_dedup_rows -------------------------------------------------------------

def ragged(seed, n=300):
    """random_requests plus empty requests (no slice; only empty slices) and
    empty slices inside others."""
    rng = np.random.default_rng(seed)
    reqs = [list(r) for r in random_requests(seed, n=n)]
    for i in rng.integers(0, n, 12):
        reqs[int(i)] = [[], [b""], [b"", b""]][int(i) % 3]
    for i in rng.integers(0, n, 12):
        reqs[int(i)] = [b""] + list(reqs[int(i)]) + [b""]
    return reqs


def check_rows(reqs, first_segment=None):
    """The properties of mirsha_dedup_rows, against mirsha_dedup_plan and a
    Python restatement over the concatenated bytes."""
    n = len(reqs)
    row, unique = dedup_rows(reqs)
    rep, unique2 = dedup_plan(reqs)
    blobs = [b"".join(bytes(s) for s in r) for r in reqs]
    assert unique == unique2 == len(set(blobs))
    assert row.dtype == np.uint32 and row.shape == (n,)
    assert np.array_equal(row, row[rep])  # row[i] == row[rep[i]]
    heads = np.flatnonzero(rep == np.arange(n))
    assert sorted(row[heads].tolist()) == list(range(unique))  # heads one-to-one onto [0, n_unique)
    where = {}
    for i, b in enumerate(blobs):  # equal bytes, equal row -- and only then
        assert where.setdefault(b, int(row[i])) == int(row[i])
    assert len(set(where.values())) == len(where)
    if first_segment is not None:
        # its heads -- the first request of each (fingerprint, length) key; with
        # weak fingerprints, of each length -- take the lowest rows, in origin order
        weak = os.environ.get("MIRSHA_AB") == "1" and os.environ.get("MIRSHA_DEDUP_WEAK_FP") == "1"
        seen, h0 = set(), []
        for i in range(first_segment):
            key = len(blobs[i]) if weak else blobs[i]
            if key not in seen:
                seen.add(key)
                h0.append(i)
        assert row[h0].tolist() == list(range(len(h0)))
        if h0 != [int(i) for i in heads if i < first_segment]:  # a collision's loser is hashed in the second launch
            assert weak and min(int(row[i]) for i in heads if i < first_segment and i not in h0) >= len(h0)
    return row


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_dedup_rows_against_python(seed):
    reqs = ragged(seed)
    row = check_rows(reqs, first_segment=len(reqs))  # one segment: rows in order of first appearance
    seen, want = {}, []
    for r in reqs:
        want.append(seen.setdefault(b"".join(bytes(s) for s in r), len(seen)))
    assert row.tolist() == want


def test_dedup_rows_small_and_invalid():
    row, u = dedup_rows([])
    assert row.size == 0 and u == 0
    row, u = dedup_rows([[b"x"]])
    assert row.tolist() == [0] and u == 1
    row, u = dedup_rows([[], [b""], [b"a", b"b"], [b"ab"], []])
    assert row.tolist() == [0, 0, 1, 1, 0] and u == 2
    lib = _lib.load()
    sl = SliceArrays.from_requests([[b"abc"], [b"abc"], [b"d"]])
    out = np.full(4, 0xA5A5A5A5, dtype=np.uint32)
    u = np.zeros(1, dtype=np.uint32)
    assert lib.mirsha_dedup_rows(sl.ptr_p, sl.len_p, sl.first_p, 3, None, u.ctypes.data_as(_lib._u32p)) \
        == _lib.MIRSHA_EINVAL
    sl.ptr[1] = 0  # a NULL slice with bytes
    assert lib.mirsha_dedup_rows(sl.ptr_p, sl.len_p, sl.first_p, 3, out.ctypes.data, None) == _lib.MIRSHA_EINVAL
    sl = SliceArrays.from_requests([[b"abc"], [b"abc"], [b"d"]])
    assert lib.mirsha_dedup_rows(sl.ptr_p, sl.len_p, sl.first_p, 3, out.ctypes.data, None) == _lib.MIRSHA_OK
    assert out.tolist() == [0, 0, 1, 0xA5A5A5A5]  # n_unique_out may be NULL; nothing past row n


@pytest.mark.parametrize("weak", [False, True])
def test_dedup_rows_in_segments(weak):
    """MIRSHA_DEDUP_SEGMENT_SLICES=5: many segments, so heads found after the
    first take the rows behind the first segment's; MIRSHA_DEDUP_WEAK_FP=1 as
    well: every same-length pair collides and is settled by the bytes."""
    code = (
        "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import numpy as np\n"
        "import test_expect_dedup_host as t\n"
        "for seed in (0, 1, 2):\n"
        "    reqs = t.ragged(seed, n=120)\n"
        "    first = np.cumsum([0] + [len(r) for r in reqs])\n"
        "    cut = next(i for i in range(1, len(reqs)) if first[i] >= 5)\n"  # DedupScan::segments' first cut
        "    row = t.check_rows(reqs, first_segment=cut)\n"
        "    assert int(row.max()) + 1 == len({b''.join(bytes(s) for s in r) for r in reqs})\n"
        # one slice each: the first segment is requests 0-4, with same-length contents in it
        "same = [[b'aa'], [b'bb'], [b'aa'], [b'cc'], [b'bb'], [b'dd'], [b'aa'], [b'x'], [b'cc']]\n"
        "row = t.check_rows(same, first_segment=5)\n"
        "assert row.tolist() == ([0, 2, 0, 3, 2, 4, 0, 1, 3] if %r else [0, 1, 0, 2, 1, 3, 0, 4, 2]), row\n"
        "print('ok')\n" % (ROOT, os.path.join(ROOT, "tests"), weak)
    )
    env = dict(os.environ, MIRSHA_AB="1", MIRSHA_DEDUP_SEGMENT_SLICES="5")
    if weak:
        env["MIRSHA_DEDUP_WEAK_FP"] = "1"
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=180)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-2000:]
