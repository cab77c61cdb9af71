"""Every class of hash_tile's tile classification, composed on purpose.

hash_tile (mirbft_amd/csrc/mirsha_kernels.hip) classifies each 64-message tile
with wave-wide predicates over its valid lanes and then takes a different
loader and a different padding path:

  far      every lane has off + 64 * wave_nb + 20 <= records, where
           records = (arena_len + 3) & ~3: plain loads; otherwise ("near") the
           range-checked 5-dword chunks
  aligned  every lane has off % 4 == 0: 4 loads per block, no fifth dword; with
           `far` also the LDS-DMA block loop (CU-block kernel, fused launch,
           split-tile block ranges) and the pipelined loop of the A/B forms
  uni      max length == min length: padding once after the transpose
           (pad_block_uniform); otherwise per-lane / per-chunk pad_words
  tail_ok  uni and at most 16 message bytes in the final block: the tail rounds
           with trimmed loads

tests/tileclasses.py builds one stream of 192 whole tiles (12,288 messages), the
product of

  lengths    u144 u128 u60 u0 (uniform, tail form: 16, 0, length-only, empty),
             u100 u93 (uniform), one_nb (56..119: one block count), one_nb_x4
             (the same, multiples of 4), mixed_nb (0..329), pad_edges (55 56 57
             63 64 65 119 120), one_long (63 x 20 bytes + one 700-byte lane:
             wave_nb far above most lanes' count), zeros_mixed (0 and 1..199)
  alignment  a16, a4 (all 16- / 4-aligned), r1, r3 (all = 1 / 3 mod 4), packed
             (back to back from an aligned base: aligned exactly when every
             length is a multiple of 4), lane0 / lane63 / lane31 (4-aligned but
             for that one lane: one lane decides the `aligned` ballot)
  placement  body (far), end (packed backward to the arena's last byte: near;
             one lane decides the `far` ballot, as the others start lower)

for arena_len % 4 in 0..3.  The tiles go to the device API in launch order with
d_order = None, so the test, not the host's bucketing, decides what each tile
holds; tests/test_tile_classes_cpu.py pins that all 16 cells of {far, near} x
{aligned, not} x {uni-tail, uni, mixed one block count, mixed} stay populated.
Aligned mixed tiles (per-lane padding in the DMA loop) are what the random
streams of test_gpu_parity.py never compose: they pack back to back, so their
offsets fall on every residue mod 4.

Expected digests come from the CPU oracle, once per stream; every comparison
is bit-exact over every message.

What a digest can and cannot pin (measured with value-logic mutants of the
kernel on an MI355X): an `aligned` ballot that loses lane 63 and a DMA loop
that pads mixed tiles with the tile's shortest length or the tile's block
count both fail here and pass the older tests.  A `far` ballot that loses
lane 63 passes everything: gfx950 range-checks the dwords of a raw buffer
load one by one, so a plain load that straddles `records` still returns the
bytes in range, and `far` chooses only between two loaders that agree.  The
end tiles still pin that both loaders are right up to the arena's last byte.
"""
import os

import numpy as np
import pytest

import oracle_py
import tileclasses as tc
from mirbft_amd import _lib
from mirbft_amd.engine import (VARIANT_CU, VARIANT_DIRECT, VARIANT_LDS, VARIANT_LDS_ONLY, VARIANT_LOWOCC,
                               VARIANT_PAIR)

pytestmark = pytest.mark.gpu

FILL = 0xA5
GUARD_ROWS = 64

_VARIANTS = [VARIANT_LDS, VARIANT_DIRECT, VARIANT_LOWOCC, VARIANT_LDS_ONLY, VARIANT_PAIR, VARIANT_CU]
_VARIANT_IDS = ["lds", "direct", "lowocc", "lds_only", "pair", "cu"]


@pytest.fixture(params=_VARIANTS, ids=_VARIANT_IDS)
def eng(engine, request):
    engine.set_variant(request.param)
    yield engine
    engine.set_variant(VARIANT_LDS)


def _torch():
    import torch

    assert torch.cuda.is_available()
    return torch


def _dev(a, view=None):
    a = np.ascontiguousarray(a)
    return _torch().from_numpy(a.view(view) if view else a).cuda()


_STREAMS = {}


def _stream(tail_mod):
    """The tile-class stream for arena_len % 4 == tail_mod: host arrays, oracle
    digests and device copies, made once per module run and never modified."""
    s = _STREAMS.get(tail_mod)
    if s is None:
        arena, off, lens, meta = tc.build(tail_mod, seed=0)
        s = dict(arena=arena, off=off, lens=lens, meta=meta, want=oracle_py.hash_requests(arena, off, lens),
                 d_arena=_dev(arena), d_off=_dev(off, np.int64), d_len=_dev(lens, np.int32))
        for a in (arena, off, lens, s["want"]):
            a.setflags(write=False)
        _STREAMS[tail_mod] = s
    return s


def _launch(engine, d_arena, arena_len, d_off, d_len, n, order=None):
    """One hash_batch_device launch into rows pre-filled with FILL; returns the
    n digest rows after checking that the rows behind them were not written."""
    torch = _torch()
    d_order = None if order is None else _dev(np.asarray(order, dtype=np.uint32), np.int32)
    d_out = torch.full((n + GUARD_ROWS, 32), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()  # torch's stream vs the engine's own (non-blocking) stream
    engine.hash_batch_device(d_arena.data_ptr(), arena_len, d_off.data_ptr(), d_len.data_ptr(),
                             None if d_order is None else d_order.data_ptr(), n, d_out.data_ptr())
    engine.sync()
    out = d_out.cpu().numpy()
    assert (out[n:] == FILL).all(), "a row past the last message was written"
    return out[:n]


def _assert_rows(got, want, meta=None, order=None):
    if np.array_equal(got, want):
        return
    bad = np.flatnonzero((got != want).any(axis=1))
    where = ""
    if meta is not None and order is None:
        tiles = sorted({int(b) // 64 for b in bad})
        where = "; tiles " + ", ".join(f"{t}={'/'.join(meta[t]) if t < len(meta) else '?'}" for t in tiles[:8])
    unwritten = int((got[bad] == FILL).all(axis=1).sum())
    raise AssertionError(f"{bad.size} of {len(want)} digests differ ({unwritten} rows unwritten), "
                         f"first messages {bad[:8].tolist()}{where}")


@pytest.mark.parametrize("tail_mod", [0, 1, 2, 3])
def test_tile_class_matrix(eng, tail_mod):
    """All 192 tiles in one launch as composed (d_order = None), then recomposed
    by a fixed permutation (msg != slot)."""
    s = _stream(tail_mod)
    n = s["lens"].size
    got = _launch(eng, s["d_arena"], s["arena"].size, s["d_off"], s["d_len"], n)
    _assert_rows(got, s["want"], s["meta"])
    order = np.random.default_rng(100 + tail_mod).permutation(n)
    got = _launch(eng, s["d_arena"], s["arena"].size, s["d_off"], s["d_len"], n, order)
    _assert_rows(got, s["want"], s["meta"], order)


_PARTIAL_TILES = [("one_nb_x4", "a4", "body"), ("mixed_nb", "a16", "end"), ("zeros_mixed", "a4", "body"),
                  ("mixed_nb", "lane0", "body"), ("one_nb_x4", "lane31", "end"), ("u100", "lane63", "body")]


@pytest.mark.parametrize("r", [1, 63])
def test_partial_last_tile(eng, r):
    """The first 64 k + r messages, with k chosen so that the partial tile is an
    aligned mixed one, then one where a single lane decides `aligned` (lane 0 is
    the only valid lane at r = 1; lanes 31 and 63 are valid or idle by r)."""
    s = _stream(1)
    for name in _PARTIAL_TILES:
        k = tc.tile_index(s["meta"], *name)
        off, lens = tc.with_partial_tile(s["off"], s["lens"], k, r)
        n = lens.size
        cls = tc.classify(off, lens, s["arena"].size)
        valid = np.arange(r)
        lane = tc.SINGLE_LANE.get(name[1], (None, 0))[0]
        assert cls["aligned"][k] == (lane is None or lane not in valid), name
        for order in (None, np.random.default_rng(7 * k + r).permutation(n)):
            got = _launch(eng, s["d_arena"], s["arena"].size, s["d_off"], s["d_len"], n, order)
            _assert_rows(got, s["want"][:n], s["meta"], order)


@pytest.fixture(scope="module")
def cus():
    return _torch().cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("spec", ["512", "513", "1024", "1025", "16cu", "16cu+1"])
def test_default_variant_routing(engine, cus, spec):
    """VARIANT_LDS picks the pair (<= 512 tiles), low-occupancy (<= 1,024),
    CU-block (<= 16 per CU) or LDS kernel by tile count: the stream repeated to
    either side of each threshold, each repetition rotated by a non-multiple
    of 64 messages so that its tiles differ from every other repetition's."""
    s = _stream(2)
    tiles = {"16cu": 16 * cus, "16cu+1": 16 * cus + 1}.get(spec) or int(spec)
    n0 = s["lens"].size
    slot = np.arange(64 * tiles)
    rep = slot // n0
    assert ((29 * np.arange(1, rep[-1] + 1)) % 64 != 0).all()
    idx = (slot + 29 * rep) % n0  # repetition j = the stream rotated by 29 j messages
    engine.set_variant(VARIANT_LDS)
    d_off, d_len = _dev(s["off"][idx], np.int64), _dev(s["lens"][idx], np.int32)
    got = _launch(engine, s["d_arena"], s["arena"].size, d_off, d_len, idx.size)
    _assert_rows(got, s["want"][idx])


_PERIOD = 1_000_003


def _aligned_irregular(seed, n=3000, n_lists=300, max_list=60, max_len=600, min_len=0):
    """test_gpu_parity's _irregular with every offset rounded up to a multiple of
    4, every third one to a multiple of 16: an aligned stream of mixed lengths."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(min_len, max_len, n).astype(np.uint32)
    # Groups of three: a 16-aligned start, then two 4-aligned ones; as every
    # start is a multiple of 4, rounding the next one up rounds the length up.
    ln = np.zeros(-(-n // 3) * 3, dtype=np.int64)
    ln[:n] = lens
    ln = ln.reshape(-1, 3)
    r4 = (ln + 3) & ~3
    base = np.concatenate([[0], np.cumsum((r4[:, 0] + r4[:, 1] + ln[:, 2] + 15) & ~15)])
    off = (base[:-1, None] + np.stack([0 * r4[:, 0], r4[:, 0], r4[:, 0] + r4[:, 1]], axis=1)).reshape(-1)[:n]
    off = off.astype(np.uint64)
    # (a random block repeated with an odd period: cheaper to draw than a large arena)
    arena = np.resize(rng.integers(0, 256, _PERIOD, dtype=np.uint8), int(base[-1]) + 1)
    sizes = rng.integers(0, max_list, n_lists)
    sizes[::9] = 0
    idx = rng.integers(0, max(n // 2, 1), int(sizes.sum())).astype(np.uint32)  # half the requests unlisted
    idx[rng.random(idx.size) < 0.1] = _lib.MIRSHA_NULL_INDEX
    first = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
    return arena, off, lens, idx, first


def _plan_runs_and_overlap(engine, plan, arena, off, lens, idx, first, want_req, want_lst, flush=False):
    """Two ordinary runs of the plan, then an overlapped cycle (two launches: the
    second hashes the first one's lists) and, if asked, the chains-only flush."""
    torch = _torch()
    n, n_lists = lens.size, first.size - 1
    d_arena, d_off, d_len = _dev(arena), _dev(off, np.int64), _dev(lens, np.int32)
    d_req = [torch.empty((n, 32), dtype=torch.uint8, device="cuda") for _ in range(2)]
    d_lst = torch.empty((max(n_lists, 1), 32), dtype=torch.uint8, device="cuda")
    args = (d_arena.data_ptr(), arena.size, d_off.data_ptr(), d_len.data_ptr())

    def refill():
        for d in d_req + [d_lst]:
            d.fill_(FILL)
        torch.cuda.synchronize()  # torch's stream vs the engine's own (non-blocking) stream

    for run in range(2):
        refill()
        engine.hash_requests_then_batches_device(plan, *args, d_req[0].data_ptr(), d_lst.data_ptr())
        plan.status()
        _assert_rows(d_req[0].cpu().numpy(), want_req)
        assert np.array_equal(d_lst.cpu().numpy()[:n_lists], want_lst), f"run {run} lists"
    refill()
    engine.pipeline_overlap_device(plan, *args, d_req[0].data_ptr(), 0, d_lst.data_ptr())
    engine.pipeline_overlap_device(plan, *args, d_req[1].data_ptr(), d_req[0].data_ptr(), d_lst.data_ptr())
    engine.sync()
    plan.status()
    _assert_rows(d_req[0].cpu().numpy(), want_req)
    _assert_rows(d_req[1].cpu().numpy(), want_req)
    assert np.array_equal(d_lst.cpu().numpy()[:n_lists], want_lst), "overlapped cycle lists"
    if flush:
        d_lst.fill_(FILL)
        torch.cuda.synchronize()
        engine.pipeline_overlap_device(plan, 0, 0, 0, 0, 0, d_req[1].data_ptr(), d_lst.data_ptr())
        engine.sync()
        plan.status()
        assert np.array_equal(d_lst.cpu().numpy()[:n_lists], want_lst), "flush lists"


_ALIGNED_PLAN = {}


def _aligned_plan_stream():
    if not _ALIGNED_PLAN:
        arena, off, lens, idx, first = _aligned_irregular(91)
        assert (off % 4 == 0).all() and (off[::3] % 16 == 0).all() and (off % 16 != 0).any()
        want_req = oracle_py.hash_requests(arena, off, lens)
        _ALIGNED_PLAN["s"] = (arena, off, lens, idx, first, want_req, oracle_py.batch_digests(want_req, idx, first))
    return _ALIGNED_PLAN["s"]


@pytest.mark.parametrize("mode,variant", [("fused", VARIANT_LDS), ("sequential", VARIANT_CU),
                                          ("sequential", VARIANT_LDS)], ids=["fused", "sequential-cu", "sequential-lds"])
def test_aligned_mixed_stream_through_plans(engine, mode, variant):
    """3,000 aligned requests of 0..599 bytes under 300 irregular lists: every
    tile aligned and mixed.  The fused launch's tile waves take the DMA loop
    with per-lane padding; the overlap kernel's tiles the register-staged
    aligned path."""
    arena, off, lens, idx, first, want_req, want_lst = _aligned_plan_stream()
    engine.set_variant(variant)
    try:
        plan = engine.pipeline(lens.size, idx, first, lens, mode=mode)
        assert plan.mode_name == mode
        _plan_runs_and_overlap(engine, plan, arena, off, lens, idx, first, want_req, want_lst)
        plan.close()
    finally:
        engine.set_variant(VARIANT_LDS)


def test_aligned_mixed_split_tiles(engine, monkeypatch):
    """More aligned mixed tiles than the fused launch has tile-wave slots: the
    overflow tiles run the DMA loop on block ranges [b0, b1) with per-lane
    padding (midstate through memory).  The smallest shape of
    test_fused_split_tiles, at 4-aligned offsets."""
    monkeypatch.setenv("MIRSHA_AB", "1")
    monkeypatch.setenv("MIRSHA_FUSED_PACE", "1")
    arena, off, lens, idx, first = _aligned_irregular(92, 64 * 1100 - 17, 2048, 60, 1300, 300)
    assert (off % 4 == 0).all()
    plan = engine.pipeline(lens.size, idx, first, lens, mode="fused")
    assert plan.mode_name == "fused"
    assert plan.split_tiles()[0] > 0, plan.split_tiles()
    want_req = oracle_py.hash_requests(arena, off, lens, threads=8)
    want_lst = oracle_py.batch_digests(want_req, idx, first)
    _plan_runs_and_overlap(engine, plan, arena, off, lens, idx, first, want_req, want_lst, flush=True)
    plan.close()


def test_host_entry_points_aligned_mixed(eng):
    """The host API composes the same class: hash_slices packs contiguously, so
    requests whose lengths are all multiples of 4 arrive aligned and mixed (a
    16-byte header plus a word-sized payload); hash_batch over the stream's
    4-aligned tiles (bucketing regroups them, every group still aligned)."""
    rng = np.random.default_rng(93)
    lens = 4 * rng.integers(0, 526, 3000)  # multiples of 4 in 0..2,100
    blob = rng.bytes(int(lens.max()) + 3000)
    msgs = [blob[i:i + int(L)] for i, L in enumerate(lens)]
    reqs = [[m[:16], m[16:]] if len(m) > 16 else [m] for m in msgs]
    _assert_rows(eng.hash_slices(reqs), oracle_py.hash_messages(msgs))
    s = _stream(3)
    cls = tc.classify(s["off"], s["lens"], s["arena"].size)
    pick = np.flatnonzero(np.repeat(cls["aligned"], 64))
    assert pick.size >= 64 * 40 and (s["off"][pick] % 4 == 0).all()
    got = eng.hash_batch(s["arena"], s["off"][pick], s["lens"][pick])
    _assert_rows(got, s["want"][pick])
