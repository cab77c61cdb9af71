"""Digest verification on the device (mirsha_verify_*): the compare kernel
through the device-pointer entry point, the three host forms on both staging
routes, the Processor's verify_on_device split and the event-log audit."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_py
from hashresult_pb import (add_results, batch_result, epoch_change_result, request_result, verify_batch_result,
                           verify_request_result)
from mirbft_amd import (Actions, HashRequest, MirshaError, Processor, SliceArrays, _lib, eventlog as el,
                        mismatch_indices)
from mirbft_amd.audit import audit_log

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCK = 256  # verify_digests_kernel: one digest per lane, 256-thread workgroups, no grid-stride loop


def _torch():
    import torch

    assert torch.cuda.is_available()
    return torch


def device_verify(engine, got, want, n=None, offset=0):
    """mirsha_verify_digests_device over host arrays; returns (bitmap words, count).
    The bitmap is pre-filled with 0xFF bytes and the count with 0xDEADBEEF."""
    torch = _torch()
    n = got.shape[0] if n is None else n
    d_got = torch.from_numpy(np.ascontiguousarray(got).reshape(-1)).cuda()
    d_want = torch.from_numpy(np.ascontiguousarray(want).reshape(-1)).cuda()
    words = (n + 63) // 64
    d_bits = torch.full((words + 1,), -1, dtype=torch.int64, device="cuda")  # one guard word
    d_count = torch.full((1,), 0xDEADBEEF - (1 << 32), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()  # torch's stream vs the engine's own (non-blocking) stream
    engine.verify_digests_device(d_got.data_ptr() + offset, d_want.data_ptr(), n, d_bits.data_ptr(),
                                 d_count.data_ptr())
    engine.sync()
    bits = d_bits.cpu().numpy().view(np.uint64)
    assert bits[words] == np.uint64(0xFFFFFFFFFFFFFFFF), "wrote past the bitmap"
    return bits[:words].copy(), int(d_count.cpu().numpy().view(np.uint32)[0])


def reference_bits(got, want):
    n = got.shape[0]
    differs = (got != want).any(axis=1)
    flags = np.zeros(((n + 63) // 64) * 64, dtype=np.uint8)
    flags[:n] = differs
    return np.packbits(flags, bitorder="little").view(np.uint64), int(differs.sum())


# One n past everything a single workgroup, a single wave and a power of two
# cover; the kernel has no grid-stride loop, so the largest size only has to
# span many workgroups and end inside a wave.
@pytest.mark.parametrize("n", [1, 63, 64, 65, 127, 128, 129, 1000, 40 * BLOCK + 37])
def test_device_compare_sizes(engine, n):
    rng = np.random.default_rng(n)
    got = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    want = got.copy()
    rows = np.flatnonzero(rng.random(n) < 0.10)
    want[rows, rng.integers(0, 32, rows.size)] ^= rng.integers(1, 256, rows.size).astype(np.uint8)
    bits, count = device_verify(engine, got, want)
    ref_bits, ref_count = reference_bits(got, want)
    assert ref_count == rows.size
    assert np.array_equal(bits, ref_bits)  # includes: bits at or beyond n are 0
    assert count == ref_count
    assert mismatch_indices(bits, n).tolist() == rows.tolist()


def test_device_compare_every_bit_counts(engine):
    n = 256
    got = np.random.default_rng(1).integers(0, 256, (n, 32), dtype=np.uint8)
    want = got.copy()
    for r in range(n):  # row r differs from its expectation in bit r alone
        want[r, r >> 3] ^= np.uint8(1 << (r & 7))
    bits, count = device_verify(engine, got, want)
    assert count == n and mismatch_indices(bits, n).tolist() == list(range(n))
    bits, count = device_verify(engine, got, got.copy())
    assert count == 0 and not bits.any()


@pytest.mark.parametrize("which", ["first", "last", "all", "alternating"])
def test_device_compare_placement(engine, which):
    n = 129
    got = np.random.default_rng(2).integers(0, 256, (n, 32), dtype=np.uint8)
    rows = {"first": [0], "last": [n - 1], "all": list(range(n)), "alternating": list(range(0, n, 2))}[which]
    want = got.copy()
    want[rows, 31] ^= 0x80
    bits, count = device_verify(engine, got, want)
    assert mismatch_indices(bits, n).tolist() == rows and count == len(rows)
    assert np.array_equal(bits, reference_bits(got, want)[0])


def test_device_compare_does_not_accumulate_and_n0(engine):
    n = 300
    got = np.random.default_rng(3).integers(0, 256, (n, 32), dtype=np.uint8)
    want = got.copy()
    want[::3, 0] ^= 1
    assert device_verify(engine, got, want)[1] == 100
    torch = _torch()
    # the same count word over two calls: mismatches, then none
    d_got = torch.from_numpy(got.reshape(-1)).cuda()
    d_bad = torch.from_numpy(want.reshape(-1)).cuda()
    d_bits = torch.zeros(5, dtype=torch.int64, device="cuda")
    d_count = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    engine.verify_digests_device(d_got.data_ptr(), d_bad.data_ptr(), n, d_bits.data_ptr(), d_count.data_ptr())
    engine.sync()
    assert int(d_count.cpu()[0]) == 100
    engine.verify_digests_device(d_got.data_ptr(), d_got.data_ptr(), n, d_bits.data_ptr(), d_count.data_ptr())
    engine.sync()
    assert int(d_count.cpu()[0]) == 0 and not d_bits.cpu().numpy().any()
    # n = 0: OK, count written as 0, bitmap untouched (NULL digests are fine)
    d_count.fill_(77)
    d_bits.fill_(-1)
    torch.cuda.synchronize()
    engine.verify_digests_device(0, 0, 0, d_bits.data_ptr(), d_count.data_ptr())
    engine.sync()
    assert int(d_count.cpu()[0]) == 0 and (d_bits.cpu().numpy() == -1).all()


def test_device_compare_rejects_misaligned_pointers(engine):
    got = np.zeros((9, 32), dtype=np.uint8)
    with pytest.raises(MirshaError) as e:
        device_verify(engine, got, got, n=8, offset=4)
    assert e.value.code == _lib.MIRSHA_EINVAL
    bits, count = device_verify(engine, got, got, n=8, offset=16)  # 16-byte aligned is enough
    assert count == 0 and not bits.any()


# ---- host forms ---------------------------------------------------------------

def random_requests(seed, n):
    """n requests of 1-3 slices, total lengths 0..600 (request 17 is empty)."""
    rng = np.random.default_rng(seed)
    reqs = []
    for i in range(n):
        total = 0 if i == 17 else int(rng.integers(0, 601))
        cuts = sorted(int(c) for c in rng.integers(0, total + 1, int(rng.integers(0, 3))))
        blob = rng.integers(0, 256, total, dtype=np.uint8).tobytes()
        reqs.append([blob[a:b] for a, b in zip([0] + cuts, cuts + [total])])
    return reqs


def oracle_slices(reqs):
    sl = SliceArrays.from_requests(reqs)
    return oracle_py.hash_slices(sl.ptr, sl.len, sl.first)


@pytest.fixture(scope="module")
def slices_case():
    reqs = random_requests(11, 600)
    assert sum(map(len, reqs[17])) == 0 and {len(r) for r in reqs} == {1, 2, 3}
    return reqs, oracle_slices(reqs)


def test_host_verify_slices(engine, slices_case):
    reqs, want = slices_case
    rng = np.random.default_rng(12)
    others = np.setdiff1d(np.arange(1, 599), [299])
    bad = sorted([0, 299, 599] + rng.choice(others, 20, replace=False).tolist())
    assert len(bad) == 23
    expected = want.copy()
    expected[bad, rng.integers(0, 32, len(bad))] ^= 0x10
    assert engine.verify_slices(reqs, want).tolist() == []
    assert engine.verify_slices(reqs, expected).tolist() == bad
    # sequence form; one expectation of 31 bytes is a mismatch by length
    seq = [bytes(r) for r in expected]
    short = next(i for i in range(600) if i not in bad)
    seq[short] = seq[short][:31]
    assert engine.verify_slices(reqs, seq).tolist() == sorted(bad + [short])
    prof = engine.host_profile()
    assert prof["chunks"] == 0 and prof["total"] > 0


def test_hash_slices_unchanged_after_verify(engine, slices_case):
    reqs, want = slices_case
    expected = want.copy()
    expected[5] ^= 0xFF
    assert engine.verify_slices(reqs, expected).tolist() == [5]
    assert np.array_equal(engine.hash_slices(reqs), want)
    assert engine.verify_slices(reqs[:0], np.empty((0, 32), dtype=np.uint8)).size == 0


def test_host_verify_batch_pipelined_route(engine):
    """140,000 x 272 B = 38 MB: over the 32 MiB staging chunk, so the call takes
    the pipelined route (chunks of 8, 16, then 32 MiB), keeps every chunk's
    digests on the device and compares once behind the last chunk."""
    n, size = 140_000, 272
    arena = oracle_py.gen_requests(0x6D69726266740002, 0, n, size - 16)
    off = np.arange(n, dtype=np.uint64) * size
    ln = np.full(n, size, dtype=np.uint32)
    want = oracle_py.hash_requests(arena, off, ln, threads=8)
    second_chunk = (8 << 20) // size  # the first request that ends beyond the first (8 MiB) chunk
    bad = [0, second_chunk, n - 1]
    expected = want.copy()
    expected[bad, 13] ^= 1
    assert engine.verify_batch(arena, off, ln, expected).tolist() == bad
    assert engine.host_profile()["chunks"] >= 2, "pipelined route not taken"
    assert engine.verify_batch(arena, off, ln, want).size == 0
    # a page-locked arena (one DMA per chunk from the caller's memory) gives the same verdict
    pinned = engine.host_empty(arena.size)
    pinned[:] = arena
    assert engine.verify_batch(pinned, off, ln, expected).tolist() == bad
    assert np.array_equal(engine.hash_batch(arena[:size * 100], off[:100], ln[:100]), want[:100])


def test_host_verify_digest_lists(engine):
    """The shape of test_device_lists_with_nulls_and_empty."""
    rng = np.random.default_rng(12)
    nd = 777
    dig = rng.integers(0, 256, (nd, 32), dtype=np.uint8)
    sizes = rng.integers(0, 45, 1500)
    sizes[::7] = 0
    idx = rng.integers(0, nd, int(sizes.sum())).astype(np.uint32)
    idx[rng.random(idx.size) < 0.15] = _lib.MIRSHA_NULL_INDEX
    first = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
    want = oracle_py.batch_digests(dig, idx, first)
    bad = [0, 7, 640, 1234, 1499]  # 0 and 7 are empty lists
    expected = want.copy()
    expected[bad, 0] ^= 0x55
    assert engine.verify_digest_lists(dig, idx, first, expected).tolist() == bad
    assert engine.verify_digest_lists(dig, idx, first, want).size == 0
    assert np.array_equal(engine.digest_lists(dig, idx, first), want)


# ---- Processor ------------------------------------------------------------------

def test_processor_verify_on_device_equals_plain(engine):
    reqs = random_requests(21, 300)
    want = oracle_slices(reqs)
    wrong = {3, 150, 297, 33}
    cycle = []
    for i, data in enumerate(reqs):
        exp = None
        if i % 3 == 0:
            exp = want[i].tobytes()
            if i in wrong:
                exp = bytes(32) if i != 33 else exp[:20]  # 33: an expectation of the wrong length
        cycle.append(HashRequest(data, ("origin", i), exp))
    assert sum(r.expected is not None for r in cycle) == 100 and all(i % 3 == 0 for i in wrong)
    plain = Processor(engine).process(Actions(hash=cycle))
    split = Processor(engine, verify_on_device=True).process(Actions(hash=cycle))
    assert [r.digest for r in plain.digests] == [want[i].tobytes() for i in range(300)]
    assert [r.digest for r in split.digests] == [r.digest for r in plain.digests]
    assert all(a.request is b.request is c for a, b, c in zip(plain.digests, split.digests, cycle))
    assert split.checkpoints == plain.checkpoints == []


# ---- audit ------------------------------------------------------------------------

def audit_events(n_events, tamper=()):
    """About n_events events holding all five HashResult kinds (request data
    retained, no empty payloads); `tamper` = (event, result) pairs whose
    recorded digest is replaced."""
    rng = np.random.default_rng(5)
    events = []
    for i in range(n_events):
        d = [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(13)]
        k = i % 5
        if k == 0:
            results = [request_result(i % 4, i, 3 * i + j, rng.integers(0, 256, int(rng.integers(1, 300)),
                                                                        dtype=np.uint8).tobytes()) for j in range(3)]
        elif k == 1:
            results = [verify_request_result(1, i, i, d[0] + d[1][:8]), batch_result(1, 2, i, [d[2], b"", d[3]])]
        elif k == 2:
            results = [verify_batch_result(2, i, d[:int(rng.integers(1, 13))])]
        elif k == 3:
            cps = [(20 * (c + 1), d[c]) for c in range(3)]
            p_set = [(6, 61 + e, d[3 + e]) for e in range(5)]
            q_set = [(6, 61 + e, d[8 + e]) for e in range(5)]
            results = [epoch_change_result(i % 4, (i + 1) % 4, 7, cps, p_set, q_set)]
        else:
            events.append(el.tick_event())
            continue
        for (ei, ri) in tamper:
            if ei == i:
                hr = results[ri]
                results[ri] = el.f_bytes(1, bytes(32)) + hr[34:]  # the recorded digest is the first field (2 + 32 bytes)
        events.append(add_results(results))
    return events


def write_log(path, events):
    with open(path, "wb") as f:
        rec = el.Recorder(1, f, time_source=lambda: 0, retain_request_data=True)
        for ev in events:
            rec.intercept(ev)
        rec.stop()


def test_audit_log_on_gpu_and_cli(engine, tmp_path):
    n = 2000
    # one result of each kind: Request, VerifyRequest, Batch, VerifyBatch, EpochChange
    tampered = [(500, 1), (1001, 0), (1501, 1), (702, 0), (1998, 0)]
    clean, bad = tmp_path / "clean.gz", tmp_path / "tampered.gz"
    write_log(clean, audit_events(n))
    write_log(bad, audit_events(n, tampered))
    with open(bad, "rb") as f:
        logged = list(el.Reader(f))
    kinds = {el.origin_hash_data(el.add_results_digests(logged[e].state_event)[r])[0] for e, r in tampered}
    assert kinds == {el.HR_REQUEST, el.HR_VERIFY_REQUEST, el.HR_BATCH, el.HR_VERIFY_BATCH, el.HR_EPOCH_CHANGE}
    rep = audit_log(logged, engine)
    assert rep.mismatches == sorted(tampered) and rep.skipped == 0 and rep.checked == 400 * (3 + 2 + 1 + 1)
    assert audit_log(logged, engine, max_bytes=50_000).mismatches == sorted(tampered)  # several device calls
    with open(clean, "rb") as f:
        assert audit_log(list(el.Reader(f)), engine).mismatches == []
    for path, code in ((bad, 1), (clean, 0)):
        r = subprocess.run([sys.executable, "-m", "mirbft_amd.audit", str(path)], cwd=ROOT, capture_output=True,
                           text=True, timeout=120)
        assert r.returncode == code, r.stderr[-2000:]
        assert ('"n_mismatch": %d' % (5 if code else 0)) in r.stdout
