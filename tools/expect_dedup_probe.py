#!/usr/bin/env python3
"""One ring ticket for a deduplicated cycle that carries expectations vs the
two submissions it replaces: one JSON line.

The cycle is config-4-shaped: 64 x 64 EpochChange acks over 64 payloads
(hashdata.epoch_change_cycle: 61,568-byte payloads of 3,847 slices, every ack
its own copy, 252 MB), followed by a run of 512 VerifyBatch requests (20 ack
digests each, batch_tracker.go:147-150) that carry matching expectations, 384
distinct and 128 of them a second copy.  Served two ways in one process
straight through the C-ABI, the legs interleaved round by round, 5 warm-up and
30 timed rounds:

  two  mirsha_submit_slices_expect on the VerifyBatch run, then
       mirsha_submit_slices(MIRSHA_SUBMIT_DEDUP) on the acks; wait for both
  one  mirsha_submit_slices_expect_dedup on the whole cycle; wait

each once with pageable and once with page-locked digest rows.  Per leg:
median / min / max of the caller-free time (the last submit has returned), of
the submit-to-wait wall time and of the ``scatter`` phase
(mirsha_ctx_host_profile, summed over the leg's tickets), the other host
phases' medians, tickets per cycle and requests hashed.  The two-submission
leg's caller would still have to stitch its two result arrays into origin
order; that is not timed.  Every round's verdict and rows are checked.

Select kernel: device time (mirsha_ctx_kernel_time id 7, one timed launch per
sample) of expect_select_kernel in the ``two`` leg and of
expect_select_gather_kernel in the ``one`` leg, in rounds of their own.

Usage (GPU box):  python tools/expect_dedup_probe.py
"""
import ctypes
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

WARM, TIMED = 5, 30
N_NODES, N_ACKS, N_VERIFY, N_VERIFY_DISTINCT, BATCH = 64, 4096, 512, 384, 20


def stats(v):
    return {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(np.min(v)), 4),
            "max_ms": round(float(np.max(v)), 4)}


def main():
    import torch

    torch.cuda.is_available()  # torch's HIP runtime first (see tests/conftest.py)
    from mirbft_amd import Engine, SliceArrays, _lib, hashdata
    from mirbft_amd.engine import KERNEL_EXPECT

    eng = Engine(0)
    lib, ctx = eng._lib, eng.ctx
    p = lambda a: a.ctypes.data if a.size else None  # noqa: E731

    # the acks, then the VerifyBatch run (each request its own copy of its bytes)
    abuf, aoff, alen, afirst, origin = hashdata.epoch_change_cycle(N_NODES, N_ACKS, 3, 640, 640)
    rng = np.random.default_rng(4)
    batches = rng.integers(0, 256, (N_VERIFY_DISTINCT, BATCH * 32), dtype=np.uint8)
    which = np.concatenate([np.arange(N_VERIFY_DISTINCT),
                            rng.integers(0, N_VERIFY_DISTINCT, N_VERIFY - N_VERIFY_DISTINCT)])
    vbuf = batches[which].reshape(-1).copy()
    voff = np.arange(N_VERIFY * BATCH, dtype=np.uint64) * 32
    vlen = np.full(N_VERIFY * BATCH, 32, dtype=np.uint64)
    vfirst = (np.arange(N_VERIFY + 1, dtype=np.uint32) * BATCH).astype(np.uint32)
    acks = SliceArrays.from_buffer(abuf, aoff, alen, afirst)
    verify = SliceArrays.from_buffer(vbuf, voff, vlen, vfirst)
    n = N_ACKS + N_VERIFY
    whole = SliceArrays(np.concatenate([acks.ptr, verify.ptr]), np.concatenate([acks.len, verify.len]),
                        np.concatenate([acks.first, verify.first[1:] + acks.first[-1]]), (acks, verify))
    plen = abuf.size // N_ACKS
    payload = [hashlib.sha256(abuf[o * plen:(o + 1) * plen].tobytes()).digest() for o in range(N_NODES)]
    want_a = np.frombuffer(b"".join(payload[o] for o in origin), dtype=np.uint8).reshape(N_ACKS, 32)
    digest = [hashlib.sha256(b.tobytes()).digest() for b in batches]
    want_v = np.frombuffer(b"".join(digest[k] for k in which), dtype=np.uint8).reshape(N_VERIFY, 32)
    of_v = np.arange(N_VERIFY, dtype=np.uint32)
    of_w = of_v + np.uint32(N_ACKS)
    rows = np.ascontiguousarray(want_v)

    outs = {"pageable": (np.empty((n, 32), np.uint8), np.empty((N_ACKS, 32), np.uint8),
                         np.empty((N_VERIFY, 32), np.uint8)),
            "pinned": (eng.host_empty(32 * n).reshape(n, 32), eng.host_empty(32 * N_ACKS).reshape(N_ACKS, 32),
                       eng.host_empty(32 * N_VERIFY).reshape(N_VERIFY, 32))}
    bits = np.zeros((n + 63) // 64, np.uint64)
    count = np.zeros(1, np.uint32)
    unique = ctypes.c_uint32(0)

    def two(kind):
        _, out_a, out_v = outs[kind]

        def call():
            out_a[:] = 0xA5
            out_v[:] = 0xA5
            t1, t2 = ctypes.c_uint64(0), ctypes.c_uint64(0)
            t0 = time.perf_counter()
            rc = lib.mirsha_submit_slices_expect(ctx, verify.ptr_p, verify.len_p, verify.first_p, N_VERIFY, p(of_v),
                                                 p(rows), N_VERIFY, p(out_v), p(bits), p(count), 0, ctypes.byref(t1))
            rc = rc or lib.mirsha_submit_slices(ctx, acks.ptr_p, acks.len_p, acks.first_p, N_ACKS, p(out_a),
                                                _lib.MIRSHA_SUBMIT_DEDUP, ctypes.byref(t2))
            free = time.perf_counter()
            rc = rc or lib.mirsha_wait(ctx, t1.value)
            prof = eng.host_profile()
            rc = rc or lib.mirsha_wait(ctx, t2.value)
            wall = time.perf_counter()
            prof2 = eng.host_profile()
            assert rc == 0, rc
            assert count[0] == 0 and np.array_equal(out_a, want_a) and (out_v == 0xA5).all()
            phases = {k: prof[k] + prof2[k] for k in prof}
            return (free - t0) * 1e3, (wall - t0) * 1e3, phases, t2.value - t1.value + 1, N_VERIFY + N_NODES
        return call

    def one(kind):
        out = outs[kind][0]

        def call():
            out[:] = 0xA5
            t = ctypes.c_uint64(0)
            t0 = time.perf_counter()
            rc = lib.mirsha_submit_slices_expect_dedup(ctx, whole.ptr_p, whole.len_p, whole.first_p, n, p(of_w),
                                                       p(rows), N_VERIFY, p(out), p(bits), p(count),
                                                       ctypes.byref(unique), ctypes.byref(t))
            free = time.perf_counter()
            rc = rc or lib.mirsha_wait(ctx, t.value)
            wall = time.perf_counter()
            assert rc == 0, rc
            assert count[0] == 0 and np.array_equal(out[:N_ACKS], want_a) and (out[N_ACKS:] == 0xA5).all()
            return (free - t0) * 1e3, (wall - t0) * 1e3, eng.host_profile(), 1, unique.value
        return call

    legs = {}
    for kind in outs:
        legs[f"two/{kind}"] = two(kind)
        legs[f"one/{kind}"] = one(kind)
    samples = {k: [] for k in legs}
    for it in range(WARM + TIMED):
        for name, call in legs.items():  # interleaved
            got = call()
            if it >= WARM:
                samples[name].append(got)
    host = {}
    for name, got in samples.items():
        host[name] = {
            "caller_free": stats([g[0] for g in got]), "wall": stats([g[1] for g in got]),
            "scatter": stats([g[2]["scatter"] for g in got]),
            "phases_median_ms": {k: round(float(np.median([g[2][k] for g in got])), 4) for k in got[0][2]},
            "tickets_per_cycle": int(got[0][3]), "requests_hashed": int(got[0][4]),
        }

    eng.set_timing(True)
    eng.set_timing_mask([KERNEL_EXPECT])
    kern = {}
    for name in ("two/pinned", "one/pinned"):
        times = []
        for it in range(WARM + TIMED):
            eng.reset_timing()
            legs[name]()
            launches, total = eng.kernel_time(KERNEL_EXPECT)
            assert launches == 1
            if it >= WARM:
                times.append(total)
        kern[name.split("/")[0]] = {"median_ms": round(float(np.median(times)), 5),
                                    "min_ms": round(float(np.min(times)), 5),
                                    "max_ms": round(float(np.max(times)), 5)}
    eng.set_timing(False)
    line = {
        "probe": "expect_dedup", "acks": N_ACKS, "payloads": N_NODES, "payload_bytes": plen,
        "verify_batches": N_VERIFY, "verify_distinct": N_VERIFY_DISTINCT, "warmup": WARM, "timed": TIMED,
        "device": torch.cuda.get_device_name(0), "legs": host, "select_kernel": kern,
        "one_over_two": {kind: {m: round(host[f"one/{kind}"][m]["median_ms"] / host[f"two/{kind}"][m]["median_ms"], 4)
                                for m in ("caller_free", "wall")} for kind in outs},
    }
    print(json.dumps(line))
    eng.close()


if __name__ == "__main__":
    main()
