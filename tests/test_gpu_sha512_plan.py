"""The device plans under the second hasher: a plan created with
mirsha_pipeline_create_hasher(..., MIRSHA_HASHER_SHA512_256) run sequentially
(mirsha_hash_requests_then_batches_device) and as an overlapped stream
(mirsha_pipeline_overlap_device), against hashlib's sha512_256 (the stand-in for
Go's sha512.New512_256), bit-exact.  The shapes are the smallest that reach
every branch of sha512_plan_lists_kernel<false / true> and of
sha512_overlap_kernel: two list workgroups, every list size around the
four-rows-a-block boundary, nulls dropped at plan creation, the last partial
batch of a uniform plan, launches with one role only."""
import hashlib

import numpy as np
import pytest

from mirbft_amd import Engine, MirshaError, _lib, sharding
from mirbft_amd.engine import KERNEL_LISTS, KERNEL_MSGS, KERNEL_OVERLAP

pytestmark = pytest.mark.gpu
NULL = _lib.MIRSHA_NULL_INDEX
LENGTHS = [0, 1, 55, 56, 111, 112, 127, 128, 129, 239, 240, 255, 256, 272, 400]
CANARY = 0xEE


def H(b) -> bytes:
    return hashlib.new("sha512_256", bytes(b)).digest()


def H256(b) -> bytes:
    return hashlib.sha256(bytes(b)).digest()


def rows(digests) -> np.ndarray:
    return np.frombuffer(b"".join(digests), dtype=np.uint8).reshape(-1, 32)


def want_requests(arena, off, ln, h=H) -> np.ndarray:
    a = bytes(arena)
    return rows([h(a[int(o): int(o) + int(k)]) for o, k in zip(off, ln)])


def want_lists(table, idx, first, h=H) -> np.ndarray:
    return rows([h(b"".join(table[i].tobytes() for i in idx[first[b]: first[b + 1]] if i != NULL))
                 for b in range(first.size - 1)])


def _torch():
    import torch

    assert torch.cuda.is_available()
    return torch


def dev(a: np.ndarray):
    return _torch().from_numpy(np.ascontiguousarray(a)).cuda()


def canary(n_rows: int):
    return _torch().full((n_rows, 32), CANARY, dtype=_torch().uint8, device="cuda")


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
    yield own
    own.set_timing(False)
    own.set_hasher("sha256")


class Cycle:
    """One cycle's requests on the device: the arena (exactly sized), its
    offsets and lengths."""

    def __init__(self, arena, off, ln):
        self.arena, self.off, self.ln = arena, off, ln
        self.n = int(off.size)
        self.d_arena = dev(arena if arena.size else np.zeros(1, dtype=np.uint8))
        self.d_off = dev(off.view(np.int64))
        self.d_len = dev(ln.view(np.int32))
        _torch().cuda.synchronize()  # torch's stream vs the engine's own (non-blocking) stream

    @property
    def args(self):
        return self.d_arena.data_ptr(), int(self.arena.size), self.d_off.data_ptr(), self.d_len.data_ptr()


def requests(rng, lengths, aligned=True):
    """Messages of `lengths`; aligned: message k starts at an offset = k mod 4."""
    off, pos = [], 0
    for k, L in enumerate(lengths):
        if aligned:
            pos += (k % 4 - pos) % 4
        off.append(pos)
        pos += int(L)
    arena = rng.integers(0, 256, size=pos, dtype=np.uint8)
    return arena, np.asarray(off, dtype=np.uint64), np.asarray(lengths, dtype=np.uint32)


def mixed_lists(rng, n_req, n_lists):
    """300 lists of 0..9 entries: every case the compaction and the block count
    c / 4 + 1 can meet (see the module's docstring and the asserts below)."""
    lists = [[], [NULL, NULL, NULL], [NULL, 5, 6], [7, NULL, 8], [9, 10, NULL], [11, 12, 11], [11, 3],
             [20, 21, 22, 23], [NULL, 24, 25, NULL, 26, 27], [30, 31, 32, 33, 34, 35, 36, 37],
             [NULL, 40, 41, 42, 43, 44, 45, 46, 47]]
    listed_below = n_req - 50  # the last 50 requests are in no list
    while len(lists) < n_lists:
        c = int(rng.integers(0, 10))
        ids = rng.integers(0, listed_below, size=c).tolist()
        for j in range(c):
            if rng.random() < 0.15:
                ids[j] = NULL
        lists.append(ids)
    idx = np.asarray([i for ids in lists for i in ids], dtype=np.uint32)
    first = np.concatenate([[0], np.cumsum([len(ids) for ids in lists])]).astype(np.uint32)
    live = [sum(i != NULL for i in ids) for ids in lists]
    assert max(len(ids) for ids in lists) <= 9 and {0, 1, 2, 3, 4, 5, 6, 7, 8} <= set(live)
    assert not (set(range(listed_below, n_req)) & set(idx.tolist()))
    return idx, first


@pytest.fixture(scope="module")
def mixed():
    """600 requests of every padding case at every byte alignment, 300 lists;
    three cycles of different bytes over the same layout.  The references
    (hashlib) are computed once and left unchanged."""
    rng = np.random.default_rng(512256)
    lengths = LENGTHS * 4 + rng.choice(LENGTHS, size=600 - 4 * len(LENGTHS)).tolist()
    arena, off, ln = requests(rng, lengths)
    assert off.size == 600 and sorted(set((off % 4).tolist())) == [0, 1, 2, 3]
    for L in LENGTHS:  # every length at every alignment
        assert {int(o) & 3 for o, k in zip(off, ln) if k == L} == {0, 1, 2, 3}, L
    idx, first = mixed_lists(rng, 600, 300)
    arenas = [arena, rng.integers(0, 256, size=arena.size, dtype=np.uint8),
              rng.integers(0, 256, size=arena.size, dtype=np.uint8)]
    req = [want_requests(a, off, ln) for a in arenas]
    bat = [want_lists(r, idx, first) for r in req]
    return dict(off=off, ln=ln, idx=idx, first=first, arenas=arenas, req=req, bat=bat)


def run_sequential(eng, plan, cyc, n_lists, slack=8):
    """One sequential run into canary-filled outputs with `slack` rows behind
    n_req / n_lists; returns (request rows, batch rows), slack included."""
    d_req, d_bat = canary(cyc.n + slack), canary(n_lists + slack)
    _torch().cuda.synchronize()
    eng.hash_requests_then_batches_device(plan, *cyc.args, d_req.data_ptr(), d_bat.data_ptr())
    eng.sync()
    return d_req.cpu().numpy(), d_bat.cpu().numpy()


# 1 ---------------------------------------------------------------------------
def test_sequential_parity_loaded_indices(eng, mixed):
    torch = _torch()
    off, ln, idx, first = mixed["off"], mixed["ln"], mixed["idx"], mixed["first"]
    n, n_lists = off.size, first.size - 1
    cyc = Cycle(mixed["arenas"][0], off, ln)
    plan = eng.pipeline(n, idx, first, ln, mode="sequential", hasher="sha512_256")
    try:
        assert plan.hasher == "sha512_256" and plan.mode_name == "sequential"
        req, bat = run_sequential(eng, plan, cyc, n_lists)
        assert np.array_equal(req[:n], mixed["req"][0])
        assert np.array_equal(bat[:n_lists], mixed["bat"][0])
        assert (req[n:] == CANARY).all() and (bat[n_lists:] == CANARY).all()
        # today's other way over the same buffers, under the same hasher: byte for byte
        d_idx, d_first = dev(idx.view(np.int32)), dev(first.view(np.int32))
        d_req2, d_bat2 = canary(n), canary(n_lists)
        torch.cuda.synchronize()
        eng.hash_batch_device(*cyc.args, None, n, d_req2.data_ptr())
        eng.digest_lists_device(d_req2.data_ptr(), n, d_idx.data_ptr(), d_first.data_ptr(), n_lists, int(idx.size),
                                d_bat2.data_ptr())
        eng.sync()
        assert d_req2.cpu().numpy().tobytes() == req[:n].tobytes()
        assert d_bat2.cpu().numpy().tobytes() == bat[:n_lists].tobytes()
    finally:
        plan.close()


# 2 ---------------------------------------------------------------------------
@pytest.mark.parametrize("n,B", [(600, 20), (601, 20), (515, 4), (514, 3), (257, 1), (3, 20)])
def test_sequential_parity_uniform_lists(eng, n, B):
    rng = np.random.default_rng(1000 * n + B)
    arena, off, ln = requests(rng, rng.integers(0, 300, size=n).tolist(), aligned=False)
    idx, first = sharding.batch_lists(n, B)
    n_lists = first.size - 1
    want_req = want_requests(arena, off, ln)
    want_bat = want_lists(want_req, idx, first)
    cyc = Cycle(arena, off, ln)
    plan = eng.pipeline(n, idx, first, ln, hasher="sha512_256")
    # each list named twice: not identity lists, so the loaded-index form
    twice = eng.pipeline(n, np.concatenate([idx, idx]), np.concatenate([first, first[1:] + first[-1]]), ln,
                         hasher="sha512_256")
    try:
        req, bat = run_sequential(eng, plan, cyc, n_lists)
        assert np.array_equal(req[:n], want_req) and np.array_equal(bat[:n_lists], want_bat)
        assert (req[n:] == CANARY).all() and (bat[n_lists:] == CANARY).all()
        req2, bat2 = run_sequential(eng, twice, cyc, 2 * n_lists)
        assert req2.tobytes() == req.tobytes()
        assert bat2[:n_lists].tobytes() == bat[:n_lists].tobytes()
        assert bat2[n_lists: 2 * n_lists].tobytes() == bat[:n_lists].tobytes()
        assert (bat2[2 * n_lists:] == CANARY).all()
    finally:
        plan.close()
        twice.close()


# 3 ---------------------------------------------------------------------------
def test_no_lists_makes_no_list_launch(eng):
    rng = np.random.default_rng(3)
    arena, off, ln = requests(rng, [272, 0, 113, 5, 128])
    cyc = Cycle(arena, off, ln)
    plan = eng.pipeline(5, np.zeros(0, dtype=np.uint32), np.zeros(1, dtype=np.uint32), ln, hasher="sha512_256")
    try:
        eng.set_timing(True)
        eng.reset_timing()
        req, bat = run_sequential(eng, plan, cyc, 0)
        assert eng.kernel_time(KERNEL_MSGS)[0] == 1 and eng.kernel_time(KERNEL_LISTS)[0] == 0
        assert np.array_equal(req[:5], want_requests(arena, off, ln))
        assert (req[5:] == CANARY).all() and (bat == CANARY).all()
    finally:
        eng.set_timing(False)
        plan.close()


@pytest.mark.parametrize("n", [1, 256, 257])
def test_request_workgroup_edges(eng, n):
    rng = np.random.default_rng(30 + n)
    arena, off, ln = requests(rng, rng.choice(LENGTHS, size=n).tolist())
    idx, first = sharding.batch_lists(n, 7)
    idx = idx[::-1].copy()  # not identity lists
    n_lists = first.size - 1
    want_req = want_requests(arena, off, ln)
    plan = eng.pipeline(n, idx, first, ln, hasher="sha512_256")
    try:
        req, bat = run_sequential(eng, plan, Cycle(arena, off, ln), n_lists)
        assert np.array_equal(req[:n], want_req) and np.array_equal(bat[:n_lists], want_lists(want_req, idx, first))
        assert (req[n:] == CANARY).all() and (bat[n_lists:] == CANARY).all()
    finally:
        plan.close()


# 4 ---------------------------------------------------------------------------
def overlapped_stream(eng, plan, cycles, want_req, want_bat, n_lists):
    """cycle 0 (tiles only), cycles 1.., the flush (chains only): after each
    call this cycle's request digests and the previous cycle's batch digests;
    exactly one launch of timing id 5 per call and none of ids 0 and 1."""
    n = cycles[0].n
    d_req = [canary(n + 8), canary(n + 8)]
    d_bat = canary(n_lists + 8)
    _torch().cuda.synchronize()
    eng.set_timing(True)
    try:
        for i in range(len(cycles) + 1):
            tiles, chains = i < len(cycles), i > 0
            prev = d_req[(i - 1) % 2].data_ptr() if chains else 0
            eng.reset_timing()
            if tiles:
                eng.pipeline_overlap_device(plan, *cycles[i].args, d_req[i % 2].data_ptr(), prev, d_bat.data_ptr())
            else:
                eng.pipeline_overlap_device(plan, 0, 0, 0, 0, 0, prev, d_bat.data_ptr())
            eng.sync()
            launches = [eng.kernel_time(k)[0] for k in (KERNEL_MSGS, KERNEL_LISTS, KERNEL_OVERLAP)]
            assert launches == [0, 0, 1], (i, launches)
            if tiles:
                got = d_req[i % 2].cpu().numpy()
                assert np.array_equal(got[:n], want_req[i]), i
                assert (got[n:] == CANARY).all(), i
            got = d_bat.cpu().numpy()
            if chains:
                assert np.array_equal(got[:n_lists], want_bat[i - 1]), i
                assert (got[n_lists:] == CANARY).all(), i
            else:
                assert (got == CANARY).all()  # a call without chains leaves the batch output alone
    finally:
        eng.set_timing(False)


def test_overlapped_stream_loaded_indices(eng, mixed):
    off, ln, idx, first = mixed["off"], mixed["ln"], mixed["idx"], mixed["first"]
    plan = eng.pipeline(off.size, idx, first, ln, hasher="sha512_256")
    try:
        cycles = [Cycle(a, off, ln) for a in mixed["arenas"]]
        overlapped_stream(eng, plan, cycles, mixed["req"], mixed["bat"], first.size - 1)
    finally:
        plan.close()


def test_overlapped_stream_uniform_lists(eng, mixed):
    off, ln = mixed["off"], mixed["ln"]
    idx, first = sharding.batch_lists(600, 20)
    plan = eng.pipeline(600, idx, first, ln, hasher="sha512_256")
    try:
        cycles = [Cycle(a, off, ln) for a in mixed["arenas"]]
        overlapped_stream(eng, plan, cycles, mixed["req"], [want_lists(r, idx, first) for r in mixed["req"]],
                          first.size - 1)
    finally:
        plan.close()


# 5 ---------------------------------------------------------------------------
def test_modes(eng):
    idx, first = sharding.batch_lists(40, 20)
    ln = np.full(40, 8, dtype=np.uint32)
    for mode in (None, "auto", "sequential"):
        plan = eng.pipeline(40, idx, first, ln, mode=mode, hasher="sha512_256")
        assert (plan.mode_name, plan.fallback, plan.hasher) == ("sequential", 0, "sha512_256"), mode
        assert plan.shape() == (0, 0, 0) and plan.split_tiles() == (0, 0) and plan.trace() is None
        plan.status()
        plan.close()
    with pytest.raises(MirshaError) as ei:
        eng.pipeline(40, idx, first, ln, mode="fused", hasher="sha512_256")
    assert ei.value.code == _lib.MIRSHA_EINVAL and "fused" in str(ei.value) and "sha512_256" in str(ei.value)
    with pytest.raises(MirshaError) as ei:
        eng.pipeline(40, idx, first, ln, hasher=7)
    assert ei.value.code == _lib.MIRSHA_EINVAL and "7" in str(ei.value)


# 6 ---------------------------------------------------------------------------
def test_guard_refuses_ahead_of_any_effect(own):
    torch = _torch()
    rng = np.random.default_rng(6)
    n = 70
    arena, off, ln = requests(rng, rng.choice(LENGTHS, size=n).tolist())
    idx, first = sharding.batch_lists(n, 6)
    idx = idx[::-1].copy()
    n_lists = first.size - 1
    cyc = Cycle(arena, off, ln)
    own.set_hasher("sha256")
    p512 = own.pipeline(n, idx, first, ln, hasher="sha512_256")  # created while the context is SHA-256
    p256 = own.pipeline(n, idx, first, ln, mode="sequential", hasher="sha256")
    try:
        d_req, d_bat = canary(n), canary(n_lists)
        torch.cuda.synchronize()
        for plan, ctx_hasher in ((p512, "sha256"), (p256, "sha512_256")):
            own.set_hasher(ctx_hasher)
            for call in (lambda: own.hash_requests_then_batches_device(plan, *cyc.args, d_req.data_ptr(),
                                                                       d_bat.data_ptr()),
                         lambda: own.pipeline_overlap_device(plan, *cyc.args, d_req.data_ptr(), d_req.data_ptr(),
                                                             d_bat.data_ptr())):
                with pytest.raises(MirshaError) as ei:
                    call()
                assert ei.value.code == _lib.MIRSHA_EINVAL
                msg = str(ei.value)  # ("sha256" is no part of "sha512_256")
                assert "sha512_256" in msg and "sha256" in msg and "mirsha_" in msg, msg
        own.sync()
        torch.cuda.synchronize()
        assert (d_req.cpu().numpy() == CANARY).all() and (d_bat.cpu().numpy() == CANARY).all()
        # matching hashers restored: the same objects give the right digests
        for plan, ctx_hasher, h in ((p512, "sha512_256", H), (p256, "sha256", H256)):
            own.set_hasher(ctx_hasher)
            req, bat = run_sequential(own, plan, cyc, n_lists, slack=0)
            want_req = want_requests(arena, off, ln, h)
            assert np.array_equal(req, want_req) and np.array_equal(bat, want_lists(want_req, idx, first, h))
    finally:
        own.set_hasher("sha256")
        p512.close()
        p256.close()


# 7 ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["sequential", "fused"])
def test_sha256_through_the_new_entry_is_create_mode(own, mixed, mode):
    off, ln, idx, first = mixed["off"], mixed["ln"], mixed["idx"], mixed["first"]
    n, n_lists = off.size, first.size - 1
    own.set_hasher("sha256")
    cyc = Cycle(mixed["arenas"][0], off, ln)
    old = own.pipeline(n, idx, first, ln, mode=mode)
    new = own.pipeline(n, idx, first, ln, mode=mode, hasher="sha256")
    try:
        assert new.hasher == old.hasher == "sha256"
        assert (new.mode, new.fallback, new.shape()) == (old.mode, old.fallback, old.shape())
        req_old, bat_old = run_sequential(own, old, cyc, n_lists)
        old.status()
        req_new, bat_new = run_sequential(own, new, cyc, n_lists)
        new.status()
        assert req_new.tobytes() == req_old.tobytes() and bat_new.tobytes() == bat_old.tobytes()
        want_req = want_requests(mixed["arenas"][0], off, ln, H256)
        assert np.array_equal(req_new[:n], want_req)
        assert np.array_equal(bat_new[:n_lists], want_lists(want_req, idx, first, H256))
    finally:
        old.close()
        new.close()


# 8 ---------------------------------------------------------------------------
def test_limits_are_refused_ahead_of_any_launch(eng):
    """No 64-bit-addressed SHA-512 form: MIRSHA_ERANGE on the host (the pointers
    are never read)."""
    idx, first = sharding.batch_lists(4, 2)
    plan = eng.pipeline(4, idx, first, np.full(4, 8, dtype=np.uint32), hasher="sha512_256")
    try:
        for call in (lambda: eng.hash_requests_then_batches_device(plan, 16, 0xFFFFFF01, 16, 16, 16, 16),
                     lambda: eng.pipeline_overlap_device(plan, 16, 0xFFFFFF01, 16, 16, 16, 16, 16)):
            with pytest.raises(MirshaError) as ei:
                call()
            assert ei.value.code == _lib.MIRSHA_ERANGE
    finally:
        plan.close()
