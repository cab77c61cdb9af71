"""Hinted uniform tiles of the request kernel, and every way a hint can be wrong.

A sequential plan created with equal lengths, and a host call whose lengths
are all equal, launch sha256_msgs_kernel with a hint (mirsha_hints.h: the one
length, the stride, the scalars that follow from the length).  Every wave
proves the hint against the lengths and offsets it loaded -- equal lengths,
off == off[lane 0] + lane * stride, 4-byte alignment, every load inside the
arena -- and takes hash_tile_uniform when the proof holds, hash_tile when it
does not (mirbft_amd/csrc/mirsha_kernels.hip).  The digests must be the
oracle's either way, so each case below is composed to land on one side of the
proof on purpose:

  correct     lengths and stride as hinted (the plan hints stride = length, so
              a length that is no multiple of 4 gets no hint there; the host
              call hints the stride of its offsets, so it does)
  nohint      the plan created without lengths
  wrong       the plan created for another length
  len_first / len_mid / len_last
              one longer message at lane 0 / 31 / the last valid lane of every wave
  gap         8 bytes more between two messages in the middle
  perm        the offsets in descending order
  overlap     stride 4 bytes short of the length (0 for lengths below 4)
  misaligned  the first offset at 1 mod 4
  arena_end   arena_len exactly the last message's end
  order       a non-identity processing order (plan: only the later half of
              the requests is listed, and listed requests go first; device
              call: an explicit reversed order)

for 1, 63, 64, 65 and 129 requests (a lone lane, a partial tile, a full one,
one lane into the second tile, a partial third) of 0, 16, 55, 56, 64, 119, 120
and 272 bytes (empty; tail form with 16 bytes; one block; a length-only final
block; tail form with 0 bytes; two blocks; ...; BASELINE config 2's request).
Each composition goes through the plan call, mirsha_hash_batch_device (never
hinted) and mirsha_hash_batch, under VARIANT_LDS_ONLY so that launches this
small reach the full-occupancy kernel.  Expected digests: the CPU oracle.
"""
import numpy as np
import pytest

import oracle_py
from mirbft_amd.engine import VARIANT_LDS, VARIANT_LDS_ONLY

pytestmark = pytest.mark.gpu

COUNTS = [1, 63, 64, 65, 129]
LENGTHS = [0, 16, 55, 56, 64, 119, 120, 272]
CASES = ["correct", "nohint", "wrong", "len_first", "len_mid", "len_last", "gap", "perm", "overlap", "misaligned",
         "arena_end", "order"]
FILL = 0xA5
SLACK = 64  # arena bytes behind the last message (none for arena_end)
_RNG_BYTES = np.random.default_rng(20260).integers(0, 256, 129 * 280 + 256, dtype=np.uint8)
_RNG_BYTES.setflags(write=False)


def _torch():
    import torch

    assert torch.cuda.is_available()
    return torch


def _dev(a, view=None):
    a = np.ascontiguousarray(a)
    return _torch().from_numpy(a.view(view) if view else a).cuda()


def compose(case, n, L):
    """(arena, off, lens, plan_len, idx, first, device_order) of one composition."""
    stride = (L + 3) & ~3
    base = 1 if case == "misaligned" else 16
    if case == "arena_end":
        base = 0
    if case == "overlap":
        stride = max(stride - 4, 0)
    off = base + stride * np.arange(n, dtype=np.int64)
    lens = np.full(n, L, dtype=np.uint32)
    lane = {"len_first": 0, "len_mid": 31, "len_last": 63}.get(case)
    if lane is not None:
        for w in range(0, n, 64):
            lens[min(w + lane, n - 1)] += 4  # (a partial wave: its last valid lane)
    if case == "gap" and n > 1:
        off[n // 2:] += 8
    if case == "perm":
        off = off[::-1].copy()
    end = int((off + lens).max())
    arena = _RNG_BYTES[: max(end, 4) if case == "arena_end" else end + SLACK]
    plan_len = {"nohint": None, "wrong": np.full(n, L + 4, dtype=np.uint32)}.get(case, np.full(n, L, dtype=np.uint32))
    if case == "order":
        idx = np.arange(n // 2, n, dtype=np.uint32)  # listed requests are processed first
        dev_order = np.arange(n, dtype=np.uint32)[::-1].copy()
    else:
        idx = np.arange(n, dtype=np.uint32)
        dev_order = None
    first = np.array([0, idx.size], dtype=np.uint32)
    return arena, off.astype(np.uint64), lens, plan_len, idx, first, dev_order


@pytest.fixture
def eng(engine):
    engine.set_variant(VARIANT_LDS_ONLY)
    yield engine
    engine.set_variant(VARIANT_LDS)


def _rows(got, want, what):
    if not np.array_equal(got, want):
        bad = np.flatnonzero((got != want).any(axis=1))
        unwritten = int((got[bad] == FILL).all(axis=1).sum())
        raise AssertionError(f"{what}: {bad.size} of {len(want)} digests differ ({unwritten} unwritten), "
                             f"first {bad[:8].tolist()}")


@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("case", CASES)
def test_hint_cases(eng, case, L):
    torch = _torch()
    for n in COUNTS:
        arena, off, lens, plan_len, idx, first, dev_order = compose(case, n, L)
        what = f"{case} n={n} L={L}"
        want = oracle_py.hash_requests(arena, off, lens)
        want_lst = oracle_py.batch_digests(want, idx, first)
        d_arena = _dev(arena) if arena.size else torch.zeros(4, dtype=torch.uint8, device="cuda")
        d_off, d_len = _dev(off, np.int64), _dev(lens, np.int32)
        d_req = torch.full((n + 1, 32), FILL, dtype=torch.uint8, device="cuda")
        d_lst = torch.full((1, 32), FILL, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()  # torch's stream vs the engine's own
        # the plan call: hinted by the lengths given at creation
        plan = eng.pipeline(n, idx, first, plan_len, mode="sequential")
        try:
            eng.hash_requests_then_batches_device(plan, d_arena.data_ptr(), arena.size, d_off.data_ptr(),
                                                  d_len.data_ptr(), d_req.data_ptr(), d_lst.data_ptr())
            eng.sync()
            plan.status()
        finally:
            plan.close()
        out = d_req.cpu().numpy()
        _rows(out[:n], want, what + " plan")
        assert (out[n:] == FILL).all(), what + ": a row past the last request was written"
        assert np.array_equal(d_lst.cpu().numpy(), want_lst), what + " plan list"
        # the device call: never hinted
        d_req.fill_(FILL)
        d_ord = None if dev_order is None else _dev(dev_order, np.int32)
        torch.cuda.synchronize()
        eng.hash_batch_device(d_arena.data_ptr(), arena.size, d_off.data_ptr(), d_len.data_ptr(),
                              None if d_ord is None else d_ord.data_ptr(), n, d_req.data_ptr())
        eng.sync()
        out = d_req.cpu().numpy()
        _rows(out[:n], want, what + " device call")
        assert (out[n:] == FILL).all(), what + ": a row past the last request was written"
        # a host call: hinted when its lengths are equal, by the stride of its offsets
        _rows(eng.hash_batch(arena, off, lens), want, what + " host call")


def test_compositions_are_what_they_claim():
    """Which side of the wave's proof each composition lands on, recomputed here
    from the arrays (no GPU work, but it belongs with the cases above)."""
    def proves(off, lens, arena_len, hint_len, hint_stride, t, n):
        lo, hi = 64 * t, min(64 * t + 64, n)
        o, ln = off[lo:hi].astype(np.int64), lens[lo:hi]
        nb = (hint_len + 72) >> 6
        u = hint_len - 64 * (nb - 1)
        reach = 64 * (nb - 1) + (16 if u > 0 else 0) if u <= 16 else 64 * nb
        records = (arena_len + 3) & ~3
        return bool((ln == hint_len).all() and (o == o[0] + hint_stride * np.arange(hi - lo)).all()
                    and o[0] % 4 == 0 and hint_stride % 4 == 0 and o[-1] + reach <= records)

    for L in LENGTHS:
        S = (L + 3) & ~3
        for n in COUNTS:
            tiles = range((n + 63) // 64)
            for case in CASES:
                arena, off, lens, _, _, _, _ = compose(case, n, L)
                got = [proves(off, lens, arena.size, L, S, t, n) for t in tiles]
                if case in ("correct", "nohint", "wrong", "order"):
                    assert all(got), (case, n, L)
                elif case == "arena_end":  # the last tile proves only when the tail form's loads end with the message
                    assert all(got[:-1]) and got[-1] == (L in (0, 16, 64, 272)), (case, n, L)
                elif case in ("len_first", "len_mid", "len_last", "misaligned"):
                    assert not any(got), (case, n, L)
                elif case == "gap" and n > 1:
                    assert not got[(n // 2) // 64] or (n // 2) % 64 == 0, (case, n, L)
                elif case == "perm" and S:  # a descending tile never proves; a lone lane has no order
                    assert got == [min(64, n - 64 * t) == 1 for t in tiles], (case, n, L)
