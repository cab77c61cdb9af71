#!/usr/bin/env python3
"""Verify on the device vs hash and ship the digests: one JSON line.

Host path: a config-2-sized call (2^20 x 272 B requests) from a page-locked
arena through mirsha_hash_batch (digests D2H, copied to the caller) and
mirsha_verify_batch (expected digests H2D, a bitmap and a count D2H), straight
through the C-ABI, interleaved A/B in one process: 5 warm-up and 30 timed
calls each, medians of a host clock around the synchronous calls, with the
library's host phases (mirsha_ctx_host_profile) of each.  verify runs twice
per round: `expected` in pageable memory (staged through the library's pinned
buffer) and in page-locked memory (DMA'd in place).  All digests match (the
common case: the count comes back 0).

Compare kernel: device time of verify_digests_kernel at n = 2^20
(mirsha_ctx_kernel_time id 6, one timed launch per sample) and the bytes/s it
implies at 64 B per digest.

Usage (GPU box):  python tools/verify_probe.py
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
    from mirbft_amd.engine import KERNEL_VERIFY

    eng = Engine(0)
    lib, ctx = eng._lib, eng.ctx
    n, stride = 1 << 20, 272
    arena = eng.host_empty(n * stride)
    arena[:] = synth.request_arena(synth.SEED_BASE + 2, 0, n, stride - 16)
    off = np.arange(n, dtype=np.uint64) * stride
    ln = np.full(n, stride, np.uint32)
    out = np.empty((n, 32), np.uint8)
    eng.hash_batch(arena, off, ln, out=out)
    expected = out.copy()
    expected_pinned = eng.host_empty(32 * n).reshape(n, 32)
    expected_pinned[:] = expected
    bits = np.zeros(n // 64, np.uint64)
    count = ctypes.c_uint32(0)
    p = lambda a: a.ctypes.data  # noqa: E731

    def hash_call():
        return lib.mirsha_hash_batch(ctx, p(arena), arena.size, p(off), p(ln), n, p(out))

    def verify_call(exp):
        return lambda: lib.mirsha_verify_batch(ctx, p(arena), arena.size, p(off), p(ln), n, p(exp), p(bits),
                                               ctypes.byref(count))

    legs = {"hash_batch": hash_call, "verify_batch": verify_call(expected),
            "verify_batch_pinned_expected": verify_call(expected_pinned)}
    ms = {k: [] for k in legs}
    prof = {k: [] for k in legs}
    for it in range(WARM + TIMED):
        for name, call in legs.items():  # interleaved
            t0 = time.perf_counter()
            rc = call()
            dt = (time.perf_counter() - t0) * 1e3
            assert rc == 0, (name, rc)
            if it >= WARM:
                ms[name].append(dt)
                prof[name].append(eng.host_profile())
        assert count.value == 0 and not bits.any()
    host = {k: {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(np.min(v)), 4),
                "phases_ms": median_profile(prof[k])} for k, v in ms.items()}

    d_got = torch.from_numpy(out.reshape(-1)).cuda()
    d_want = torch.from_numpy(expected.reshape(-1)).cuda()
    d_bits = torch.zeros(n // 64, dtype=torch.int64, device="cuda")
    d_count = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    eng.set_timing(True)
    eng.set_timing_mask([KERNEL_VERIFY])
    kern = []
    for it in range(WARM + TIMED):
        eng.reset_timing()
        eng.verify_digests_device(d_got.data_ptr(), d_want.data_ptr(), n, d_bits.data_ptr(), d_count.data_ptr())
        launches, total = eng.kernel_time(KERNEL_VERIFY)
        assert launches == 1
        if it >= WARM:
            kern.append(total)
    eng.set_timing(False)
    k_ms = float(np.median(kern))
    line = {
        "probe": "verify", "n": n, "request_bytes": stride, "warmup": WARM, "timed": TIMED,
        "device": torch.cuda.get_device_name(0), "host_path": host,
        "verify_over_hash": round(host["verify_batch"]["median_ms"] / host["hash_batch"]["median_ms"], 4),
        "d2h_bytes": {"hash_batch": 32 * n, "verify_batch": 8 + 8 * (n // 64)},
        "compare_kernel": {"median_ms": round(k_ms, 5), "min_ms": round(float(np.min(kern)), 5),
                           "gb_per_s": round(64 * n / k_ms / 1e6, 1)},
    }
    print(json.dumps(line))
    eng.close()


if __name__ == "__main__":
    main()
