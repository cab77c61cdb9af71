#!/usr/bin/env python3
"""Mixed hash-and-verify ring submissions vs the plain ring submission: one JSON line.

A config-2-sized cycle (2^20 x 272 B requests) in a page-locked arena, straight
through the C-ABI, interleaved legs in one process: 5 warm-up and 30 timed
rounds, medians of a host clock around submit + wait, with the library's host
phases (mirsha_ctx_host_profile) of each.  Legs: mirsha_submit_batch, and
mirsha_submit_batch_expect with 0 %, 50 % (every other request) and 100 % of
the requests carrying a matching expectation; each once with a pageable and
once with a page-locked digests_out (the kernels store into the latter).

Select kernel: device time of expect_select_kernel (mirsha_ctx_kernel_time id
7, one timed launch per sample) in the 50 % and 100 % legs, measured in rounds
of their own after the host-clock rounds.

Usage (GPU box):  python tools/expect_probe.py
"""
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests", "golden")]
import synth  # noqa: E402

WARM, TIMED = 5, 30


def median_profile(profiles):
    return {k: round(float(np.median([p[k] for p in profiles])), 4) for k in profiles[0]}


def main():
    import torch

    torch.cuda.is_available()  # torch's HIP runtime first (see tests/conftest.py)
    from mirbft_amd import Engine
    from mirbft_amd.engine import KERNEL_EXPECT

    eng = Engine(0)
    lib, ctx = eng._lib, eng.ctx
    n, stride = 1 << 20, 272
    arena = eng.host_empty(n * stride)
    arena[:] = synth.request_arena(synth.SEED_BASE + 2, 0, n, stride - 16)
    off = np.arange(n, dtype=np.uint64) * stride
    ln = np.full(n, stride, np.uint32)
    want = eng.hash_batch(arena, off, ln)
    outs = {"pageable": np.empty((n, 32), np.uint8), "pinned": eng.host_empty(32 * n).reshape(n, 32)}
    bits = np.zeros(n // 64, np.uint64)
    count = np.zeros(1, np.uint32)
    p = lambda a: a.ctypes.data if a.size else None  # noqa: E731
    plans = {}
    for pct, step in ((0, 0), (50, 2), (100, 1)):
        of = np.arange(0, n, step, dtype=np.uint32) if step else np.zeros(0, np.uint32)
        plans[pct] = (of, np.ascontiguousarray(want[of]))

    def plain(out):
        def call():
            t = ctypes.c_uint64(0)
            rc = lib.mirsha_submit_batch(ctx, p(arena), arena.size, p(off), p(ln), n, p(out), ctypes.byref(t))
            return rc or lib.mirsha_wait(ctx, t.value)
        return call

    def expect(out, pct):
        of, rows = plans[pct]

        def call():
            t = ctypes.c_uint64(0)
            rc = lib.mirsha_submit_batch_expect(ctx, p(arena), arena.size, p(off), p(ln), n, p(of), p(rows), of.size,
                                                p(out), p(bits), p(count), ctypes.byref(t))
            return rc or lib.mirsha_wait(ctx, t.value)
        return call

    legs = {}
    for kind, out in outs.items():
        legs[f"submit_batch/{kind}"] = plain(out)
        for pct in plans:
            legs[f"expect_{pct}/{kind}"] = expect(out, pct)
    ms = {k: [] for k in legs}
    prof = {k: [] for k in legs}
    for it in range(WARM + TIMED):
        for name, call in legs.items():  # interleaved
            t0 = time.perf_counter()
            rc = call()
            dt = (time.perf_counter() - t0) * 1e3
            assert rc == 0, (name, rc)
            assert count[0] == 0 and not bits.any()
            if it >= WARM:
                ms[name].append(dt)
                prof[name].append(eng.host_profile())
    host = {k: {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(np.min(v)), 4),
                "phases_ms": median_profile(prof[k])} for k, v in ms.items()}
    for out in outs.values():  # every row came from the plain and 0 % legs; the 100 % leg writes none
        assert np.array_equal(out, want)

    eng.set_timing(True)
    eng.set_timing_mask([KERNEL_EXPECT])
    kern = {}
    for pct in (50, 100):
        call, samples = expect(outs["pinned"], pct), []
        for it in range(WARM + TIMED):
            eng.reset_timing()
            assert call() == 0
            launches, total = eng.kernel_time(KERNEL_EXPECT)
            assert launches == 1
            if it >= WARM:
                samples.append(total)
        kern[f"expect_{pct}"] = {"median_ms": round(float(np.median(samples)), 5),
                                 "min_ms": round(float(np.min(samples)), 5)}
    eng.set_timing(False)
    base = {kind: host[f"submit_batch/{kind}"]["median_ms"] for kind in outs}
    line = {
        "probe": "expect", "n": n, "request_bytes": stride, "warmup": WARM, "timed": TIMED,
        "device": torch.cuda.get_device_name(0), "legs": host,
        "over_submit_batch": {k: round(v["median_ms"] / base[k.split("/")[1]], 4) for k, v in host.items()},
        "select_kernel": kern,
    }
    print(json.dumps(line))
    eng.close()


if __name__ == "__main__":
    main()
