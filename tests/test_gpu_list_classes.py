"""Every class of the dependent pass's wave-wide decisions, composed on purpose.

The dependent pass (batch, VerifyBatch and checkpoint-list digests over
request digests) has six forms in mirbft_amd/csrc/mirsha_kernels.hip:
sha256_lists_kernel (optimistic hash_list, a wave-wide null ballot, compaction
into scratch and a second pass), sha256_chain_pair_kernel (pair_loop),
sha256_chain_kernel<false> (loaded bounds and indices) and <true> (computed
ones, with the constant-schedule block of a pad_wave), overlap_chain, and
fused_list_produce / fused_list_consume.  The first four walk their lists
through the one prefetching source, ListBlocks (loaded or computed indices,
the null report switched on for the lists kernel alone); the last two keep
load schedules of their own.  All six build a block with list_block_words
(mirsha_device.h).  Each gives one lane a list, decides with predicates over
64 lists (null ballot, wave_max of the block counts, pad_wave), pads by
`ordinal == c` on zero-filled range-checked loads, and reads indices through
a descriptor that ends exactly at n_entries.

tests/listclasses.py builds one stream of 273 whole groups (17,472 lists) over
1,024 digests, the product of

  counts   u0 u1 u2 u3 u4 u5 u8 u9 (all 64 alike: marker parity, the
           padding-only block, the 4-digest chunk edge of the fused producer,
           the prefetch depths), edges (0..9 over the lanes), one_long (63 x 2
           and one list of 41: wave_nb far above most lanes'), mixed (0..44),
           zeros_mixed (every other lane empty), one_nb (2 or 3: two counts,
           one block count)
  nulls    none, lane0_first, lane63_last (one lane decides the ballot, the
           compacted parity flips), lane31_all (compacts to the empty
           message), each_one (positions 2..5, the prefetched entries, among
           them), half, all_null
  indices  distinct, edge (first live entry 0, last n_digests - 1, the last
           row the digest descriptor admits), shared (all lanes one sequence)

and tests/test_list_classes_cpu.py pins that every cell of the raw view (what
the lists kernel sees) and of the compacted view (what every plan form sees)
stays populated, and that the thresholds restated there equal the header's.
The forms are reached on purpose: the lists kernel through the device and
host entry points; the pair kernel by the stream as composed; the chain
kernel, which runs in-process only above 512 groups, by the stream repeated
to 513 groups, each repetition rotated by a non-multiple of 64 lists;
overlap_chain by overlapped cycles and the chains-only flush of those plans;
the fused pair by a fused plan whose shape() must equal the classification's
counts; sha256_chain_kernel<true> by identity lists on both sides of the
threshold with full, short and partial last waves.

Expected digests come from the CPU oracle, once per stream; every output
buffer is pre-filled and has guard rows behind it; every comparison is
bit-exact over every list and names the recipes of the groups that differ.

That these tests can fail (measured once with value-logic mutants of the
kernels on an MI355X; none committed): a null ballot in sha256_lists_kernel
that loses lane 63, and a hash_list whose saw_null looks at the first two
entries only and not at the prefetched ones, both fail the six lists-kernel
tests here (the lane63_last groups; each_one keeps its nulls behind entry 1
for the same reason) and pass every older list test, whose random streams put
a null in practically every wave.  A pad_wave taken with __any instead of
__all fails test_identity_lists for every even B at 513 x 64 and 513 x 64 + 63
lists, a short last list beside full ones; an overlap_chain that takes wave_nb
from lane 0 fails all of test_sequential_plans_routed; a loaded-index chain
kernel that does the same fails only its 513-group case.  The older
BatchSize and irregular streams catch these three as well.  (The mutants were
of the kernels as they stood before ListBlocks became the one list source; the
predicates they broke are the same.)
"""
import hashlib

import numpy as np
import pytest

import listclasses as lc
import oracle_py

pytestmark = pytest.mark.gpu

FILL = 0xA5
GUARD_ROWS = 64
EMPTY = np.frombuffer(hashlib.sha256(b"").digest(), dtype=np.uint8)


def _torch():
    import torch

    assert torch.cuda.is_available()
    return torch


def _dev(a, view=None):
    a = np.ascontiguousarray(a)
    return _torch().from_numpy(a.view(view) if view else a).cuda()


def _requests(seed, n, max_len):
    """n short requests of mixed lengths, packed: host arrays, oracle digests and
    device copies."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, max_len, n).astype(np.uint32)
    off = np.zeros(n, dtype=np.uint64)
    np.cumsum(lens[:-1], out=off[1:])
    arena = rng.integers(0, 256, int(lens.sum()) + 1, dtype=np.uint8)
    r = dict(n=n, arena=arena, off=off, lens=lens, want_req=oracle_py.hash_requests(arena, off, lens, threads=8),
             d_arena=_dev(arena), d_off=_dev(off, np.int64), d_len=_dev(lens, np.int32))
    for a in (arena, off, lens, r["want_req"]):
        a.setflags(write=False)
    return r


_CACHE = {}


def _stream():
    """The list-class stream over the digests of 1,024 short requests: made once
    per module run and never modified."""
    s = _CACHE.get("stream")
    if s is None:
        idx, first, n_digests, meta = lc.build(seed=0)
        s = _requests(81, n_digests, 48)
        s.update(idx=idx, first=first, meta=meta, n_lists=first.size - 1, cls=lc.classify(idx, first),
                 want_lst=oracle_py.batch_digests(s["want_req"], idx, first),
                 d_idx=_dev(idx, np.int32), d_first=_dev(first, np.int32), d_dig=_dev(s["want_req"].copy()))
        for a in (idx, first, s["want_lst"]):
            a.setflags(write=False)
        _CACHE["stream"] = s
    return s


def _assert_lists(got, want, what, meta=None, src=None):
    if np.array_equal(got, want):
        return
    bad = np.flatnonzero((got != want).any(axis=1))
    where = ""
    if meta is not None:
        lists = bad if src is None else np.asarray(src)[bad]
        names = []
        for g in (lists // 64).tolist():
            if "/".join(meta[g]) not in names:
                names.append("/".join(meta[g]))
        where = f"; recipes ({len(names)}) " + ", ".join(names[:12])
    unwritten = int((got[bad] == FILL).all(axis=1).sum())
    raise AssertionError(f"{what}: {bad.size} of {len(want)} list digests differ ({unwritten} rows unwritten), "
                         f"first lists {bad[:8].tolist()}{where}")


def _rows(d_out, n, what):
    """The n rows of a pre-filled device buffer after checking its guard rows."""
    out = d_out.cpu().numpy()
    assert (out[n:] == FILL).all(), f"{what}: a row past the last one was written"
    return out[:n]


def _filled(rows):
    return _torch().full((rows + GUARD_ROWS, 32), FILL, dtype=_torch().uint8, device="cuda")


# ---- 1. the lists kernel through the device API -----------------------------


def _lists_device(engine, s, n_lists, n_entries):
    torch = _torch()
    d_out = _filled(n_lists)
    torch.cuda.synchronize()  # torch's stream vs the engine's own (non-blocking) stream
    engine.digest_lists_device(s["d_dig"].data_ptr(), s["n"], s["d_idx"].data_ptr(), s["d_first"].data_ptr(), n_lists,
                               n_entries, d_out.data_ptr())
    engine.sync()
    return _rows(d_out, n_lists, "digest_lists_device")


def test_lists_kernel_whole_stream(engine):
    """All 273 groups in one launch: a workgroup's four waves are four
    consecutive groups, so optimistic-only waves run beside compacting ones.
    Compaction writes scratch, never idx."""
    s = _stream()
    got = _lists_device(engine, s, s["n_lists"], s["idx"].size)
    _assert_lists(got, s["want_lst"], "whole stream", s["meta"])
    assert np.array_equal(s["d_idx"].cpu().numpy().view(np.uint32), s["idx"]), "the device copy of idx was modified"


@pytest.mark.parametrize("r", [1, 63])
def test_lists_kernel_partial_last_wave(engine, r):
    """The stream cut to the first r lists of a named group: n_entries, and with
    it the descriptor of idx, ends behind lists of 0, 1, 2 and 3 entries; lane
    0 is the only valid lane at r = 1, lane 63 is idle at both r."""
    s = _stream()
    for name in lc.PARTIAL_GROUPS:
        g = lc.group_index(s["meta"], *name)
        _, f = lc.with_partial_group(s["first"], s["idx"], g, r)
        n = f.size - 1
        got = _lists_device(engine, s, n, int(f[-1]))
        _assert_lists(got, s["want_lst"][:n], f"prefix ending in {r} lists of {'/'.join(name)}", s["meta"])


# ---- 2. host entry points -----------------------------------------------------


def test_digest_lists_host(engine):
    s = _stream()
    got = engine.digest_lists(s["want_req"], s["idx"], s["first"])
    _assert_lists(got, s["want_lst"], "digest_lists", s["meta"])


def test_verify_digest_lists_host(engine):
    """The oracle's digests as expectations, a few rows flipped by one bit:
    exactly those rows are reported."""
    s = _stream()
    meta, n = s["meta"], s["n_lists"]
    flipped = sorted({0, 63, 64, n - 1, n // 2 + 17,
                      64 * lc.group_index(meta, "u0", "none", "distinct") + 5,
                      64 * lc.group_index(meta, "mixed", "all_null", "edge") + 31,
                      64 * lc.group_index(meta, "u3", "lane63_last", "shared") + 63})
    exp = s["want_lst"].copy()
    for j, k in enumerate(flipped):
        exp[k, (5 * j) % 32] ^= 1 << (j % 8)
    bad = engine.verify_digest_lists(s["want_req"], s["idx"], s["first"], exp)
    assert bad.tolist() == flipped
    assert engine.verify_digest_lists(s["want_req"], s["idx"], s["first"], s["want_lst"]).size == 0


def test_hash_requests_then_batches_general_path(engine, monkeypatch):
    """The host call without a plan (MIRSHA_PIPELINE_MODE unset): the request
    kernel, then the lists kernel over its digests on the device."""
    monkeypatch.delenv("MIRSHA_PIPELINE_MODE", raising=False)
    s = _stream()
    req = np.full((s["n"] + GUARD_ROWS, 32), FILL, dtype=np.uint8)
    bat = np.full((s["n_lists"] + GUARD_ROWS, 32), FILL, dtype=np.uint8)
    engine.hash_requests_then_batches(s["arena"], s["off"], s["lens"], s["idx"], s["first"], out=req[:s["n"]],
                                      batch_out=bat[:s["n_lists"]])
    assert (req[s["n"]:] == FILL).all() and (bat[s["n_lists"]:] == FILL).all()
    assert np.array_equal(req[:s["n"]], s["want_req"])
    _assert_lists(bat[:s["n_lists"]], s["want_lst"], "hash_requests_then_batches", s["meta"])


# ---- 3. to 5. plans -----------------------------------------------------------


def _plan_cycle(engine, plan, r, n_lists, want_lst, meta=None, src=None, overlap=True):
    """Two ordinary runs of the plan, an overlapped cycle (two launches: the
    second hashes the first one's lists) unless overlap is False, and the
    chains-only flush; every launch into pre-filled, guarded buffers."""
    torch = _torch()
    n = r["n"]
    d_req = [_filled(n) for _ in range(2)]
    d_lst = _filled(n_lists)
    args = (r["d_arena"].data_ptr(), r["arena"].size, r["d_off"].data_ptr(), r["d_len"].data_ptr())

    def refill(bufs):
        for d in bufs:
            d.fill_(FILL)
        torch.cuda.synchronize()  # torch's stream vs the engine's own (non-blocking) stream

    def check(what, reqs):
        for d in reqs:
            assert np.array_equal(_rows(d, n, what), r["want_req"]), f"{what}: request digests differ"
        _assert_lists(_rows(d_lst, n_lists, what), want_lst, what, meta, src)

    for run in range(2):
        refill(d_req + [d_lst])
        engine.hash_requests_then_batches_device(plan, *args, d_req[0].data_ptr(), d_lst.data_ptr())
        plan.status()
        check(f"ordinary run {run}", d_req[:1])
    if overlap:
        refill(d_req + [d_lst])
        engine.pipeline_overlap_device(plan, *args, d_req[0].data_ptr(), 0, d_lst.data_ptr())
        engine.pipeline_overlap_device(plan, *args, d_req[1].data_ptr(), d_req[0].data_ptr(), d_lst.data_ptr())
        engine.sync()
        plan.status()
        check("overlapped cycle", d_req)
    refill([d_lst])
    engine.pipeline_overlap_device(plan, 0, 0, 0, 0, 0, d_req[0].data_ptr(), d_lst.data_ptr())
    engine.sync()
    plan.status()
    check("chains-only flush", [])


@pytest.mark.parametrize("groups", [273, lc.K_PAIR_MAX_GROUPS, lc.K_PAIR_MAX_GROUPS + 1])
def test_sequential_plans_routed(engine, groups):
    """273 groups (the stream as composed) and 512: sha256_chain_pair_kernel;
    513, the smallest plan at which it runs in-process: sha256_chain_kernel
    <false>.  The overlapped cycle and the flush of each run overlap_chain."""
    s = _stream()
    if groups == len(s["meta"]):
        idx, first, src, want = s["idx"], s["first"], None, s["want_lst"]
    else:
        idx, first, src = lc.repeat_rotated(s["idx"], s["first"], groups)
        want = s["want_lst"][src]
    n_lists = first.size - 1
    assert (n_lists + 63) // 64 == groups
    plan = engine.pipeline(s["n"], idx, first, s["lens"], mode="sequential")
    assert plan.mode_name == "sequential"
    _plan_cycle(engine, plan, s, n_lists, want, s["meta"], src)
    plan.close()


def test_fused_plan(engine):
    """The composed stream on a fused plan: two ordinary runs (readiness waits),
    an overlapped cycle (no waits) and the flush (pair kernel).  A plan has at
    most min(n_groups, kFusedMaxListBlocks = 32, cus / 8) list blocks, fewer
    than the 273 groups on any MI355X, so every producer / consumer pair takes
    several groups in turn, groups of odd and even wave_nb follow each other on
    one pair, and the ring slot parity `seq & 1` carries over from group to
    group.  shape() and the classification pin each other."""
    s = _stream()
    plan = engine.pipeline(s["n"], s["idx"], s["first"], s["lens"], mode="fused")
    assert plan.mode_name == "fused"
    assert plan.shape() == ((s["n"] + 63) // 64, int(s["cls"]["chunks"].sum()), len(s["meta"]))
    _plan_cycle(engine, plan, s, s["n_lists"], s["want_lst"], s["meta"])
    plan.status()
    plan.close()


@pytest.mark.parametrize("mode", ["sequential", "fused"])
@pytest.mark.parametrize("kind", ["empty", "all_null"])
def test_nothing_to_hash(engine, mode, kind):
    """130 lists that are all empty or all null: n_entries == 0 after the host's
    compaction, so the index descriptor admits nothing, every list is the
    padding block alone and every row the empty-message digest.  (Fused: the
    producer's readiness target is epoch x expected = 0, so it never waits.)"""
    s = _stream()
    n_lists = 130
    counts = np.zeros(n_lists, dtype=np.int64) if kind == "empty" else np.arange(n_lists) % 7
    first = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
    idx = np.full(int(first[-1]), lc.K_NULL_INDEX, dtype=np.uint32)
    cls = lc.classify(idx, first)
    assert (cls["wave_nb"] == 1).all() and cls["has_empty"].all()
    plan = engine.pipeline(s["n"], idx, first, s["lens"], mode=mode)
    assert plan.mode_name == mode
    if mode == "fused":
        assert plan.shape() == ((s["n"] + 63) // 64, 3, 3)
    _plan_cycle(engine, plan, s, n_lists, np.tile(EMPTY, (n_lists, 1)), overlap=False)
    plan.close()


# ---- 6. identity lists on both sides of both thresholds ------------------------

_GROUPS = lc.K_PAIR_MAX_GROUPS
_N_LISTS = {"512x64": _GROUPS * 64, "513x64": (_GROUPS + 1) * 64, "513x64+1": (_GROUPS + 1) * 64 + 1,
            "513x64+63": (_GROUPS + 1) * 64 + 63}
_MAX_B = 20


def _tiny_requests():
    r = _CACHE.get("tiny")
    if r is None:
        r = _CACHE["tiny"] = _requests(82, max(_N_LISTS.values()) * _MAX_B, 8)  # 0..7 bytes each
        r["d_req"], r["d_lst"] = _filled(r["n"]), _filled(max(_N_LISTS.values()))
    return r


@pytest.mark.parametrize("spec", list(_N_LISTS))
@pytest.mark.parametrize("B", [1, 2, 3, 4, _MAX_B])
def test_identity_lists(engine, B, spec):
    """uniform(n, B) on sequential plans: 512 x 64 lists run the pair kernel,
    513 x 64 and more sha256_chain_kernel<true>.  The last list is full, one
    short of full, or a single digest.  With an even B that gives: every wave
    a pad_wave, a full last wave included (513 x 64, full); a full last wave
    that is none, because its last list is short (513 x 64, short); a partial
    last wave, whose idle lanes must not vote (513 x 64 + 1, + 63)."""
    torch = _torch()
    r = _tiny_requests()
    n_lists = _N_LISTS[spec]
    for last in sorted({B, max(B - 1, 1), 1}):
        n = (n_lists - 1) * B + last
        idx, first = lc.uniform(n, B)
        assert first.size - 1 == n_lists and first[-1] - first[-2] == last
        want_req = r["want_req"][:n]
        want_lst = oracle_py.batch_digests(want_req, idx, first)
        plan = engine.pipeline(n, idx, first, r["lens"][:n], mode="sequential")
        assert plan.mode_name == "sequential"
        for run in range(2):
            what = f"B = {B}, {spec} lists, last list of {last}, run {run}"
            r["d_req"].fill_(FILL)
            r["d_lst"].fill_(FILL)
            torch.cuda.synchronize()  # torch's stream vs the engine's own (non-blocking) stream
            engine.hash_requests_then_batches_device(plan, r["d_arena"].data_ptr(), r["arena"].size,
                                                     r["d_off"].data_ptr(), r["d_len"].data_ptr(),
                                                     r["d_req"].data_ptr(), r["d_lst"].data_ptr())
            plan.status()
            if run == 0:
                assert np.array_equal(_rows(r["d_req"], n, what), want_req), f"{what}: request digests differ"
            _assert_lists(_rows(r["d_lst"], n_lists, what), want_lst, what)
        plan.close()
