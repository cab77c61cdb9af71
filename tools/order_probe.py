#!/usr/bin/env python3
"""The bucket order built on the device vs on the host: one JSON line.

One process, legs interleaved round by round, 5 warm-up and 30 timed rounds,
medians with min-max; every round's result is checked.

Leg (a), the sort alone, n = 2^20 lengths already on the device, two length
sets (uniform 80-616 B: 9 block counts; log-uniform 64 B-64 KB: 1,024):
  host    mirsha_bucket_order on this box's host, one thread (host clock)
  device  mirsha_bucket_order_device: host clock around the call and a stream
          synchronisation (queueing, the three launches, the wake-up), and in
          rounds of their own the device time of the count and scatter kernels
          (mirsha_ctx_kernel_time id 8; rocPRIM's scan between them is not in it)

Leg (b), a whole cycle through mirsha_submit_batch, page-locked arena and
digests_out, MIRSHA_ORDER_HOST against MIRSHA_ORDER_DEVICE:
  2^20 requests of 80-616 B (gapless, ~365 MB)
  2^17 requests, log-uniform 64 B-64 KB (gapless, ~1.2 GB)
submit = the call returns (the caller is free), wall = submit to mirsha_wait
returning, and the library's host phases of the ticket (mirsha_ctx_host_profile).

Usage (GPU box):  python tools/order_probe.py
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


def stats(v):
    return {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(np.min(v)), 4),
            "max_ms": round(float(np.max(v)), 4)}


def length_sets(n_uniform, n_log):
    rng = np.random.default_rng(20)
    uniform = rng.integers(80, 617, n_uniform).astype(np.uint32)
    log = np.exp(rng.uniform(np.log(64.0), np.log(65536.0), n_log)).astype(np.uint32)
    log = np.clip(log, 64, 65536).astype(np.uint32)
    log[:2] = (64, 65536)
    return {"uniform_80_616": (uniform, 80, 616), "loguniform_64_64k": (log, 64, 65536)}


def sort_leg(eng, torch):
    from mirbft_amd import bucket_order, order_plan
    from mirbft_amd.engine import KERNEL_ORDER

    n = 1 << 20
    out = {}
    for name, (lens, lo, hi) in length_sets(n, n).items():
        d_len = torch.from_numpy(lens.view(np.int32)).cuda()
        d_ord = torch.empty(n, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        want, _ = bucket_order(lens)
        order = np.empty(n, dtype=np.uint32)
        lib = eng._lib
        host, dev = [], []
        for it in range(WARM + TIMED):
            t0 = time.perf_counter()
            lib.mirsha_bucket_order(lens.ctypes.data, n, order.ctypes.data)
            t1 = time.perf_counter()
            eng.bucket_order_device(d_len.data_ptr(), n, lo, hi, d_ord.data_ptr())
            eng.sync()
            t2 = time.perf_counter()
            assert np.array_equal(d_ord.cpu().numpy().view(np.uint32), want) and np.array_equal(order, want)
            if it >= WARM:
                host.append((t1 - t0) * 1e3)
                dev.append((t2 - t1) * 1e3)
        eng.set_timing(True)
        eng.set_timing_mask([KERNEL_ORDER])
        kern = []
        for it in range(WARM + TIMED):
            eng.reset_timing()
            eng.bucket_order_device(d_len.data_ptr(), n, lo, hi, d_ord.data_ptr())
            launches, total = eng.kernel_time(KERNEL_ORDER)
            assert launches == 2
            if it >= WARM:
                kern.append(total)
        eng.set_timing(False)
        eng.set_timing_mask(range(9))
        bins, chunk, n_chunks, scratch = order_plan(n, lo, hi)
        out[name] = {"n": n, "bins": bins, "chunk": chunk, "waves": n_chunks, "scratch_bytes": scratch,
                     "host_sort": stats(host), "device_call_and_sync": stats(dev),
                     "count_and_scatter_kernels": stats(kern)}
    return out


def cycle_leg(eng):
    sets = length_sets(1 << 20, 1 << 17)
    lib, ctx = eng._lib, eng.ctx
    out = {}
    for name, (lens, _, _) in sets.items():
        n = lens.size
        off = np.zeros(n, dtype=np.uint64)
        np.cumsum(lens[:-1], dtype=np.uint64, out=off[1:])
        total = int(off[-1]) + int(lens[-1])
        arena = eng.host_empty(total)
        block = np.random.default_rng(21).integers(0, 256, 1 << 24, dtype=np.uint8)
        for a in range(0, total, block.size):
            arena[a:a + block.size] = block[:min(block.size, total - a)]
        arena[off.astype(np.int64)[lens > 0]] = (np.arange(n)[lens > 0] & 0xFF).astype(np.uint8)  # no two alike
        digests = eng.host_empty(32 * n).reshape(n, 32)
        eng.set_order_mode("host")
        want = eng.hash_batch(arena, off, lens)
        for i in np.random.default_rng(22).choice(n, 64, replace=False):  # the reference against hashlib
            m = arena[int(off[i]):int(off[i]) + int(lens[i])].tobytes()
            assert want[i].tobytes() == hashlib.sha256(m).digest()
        ms = {m: {"submit": [], "wall": []} for m in ("host", "device")}
        prof = {m: [] for m in ms}
        for it in range(WARM + TIMED):
            for mode in ms:  # interleaved
                eng.set_order_mode(mode)
                digests[:] = 0
                t = ctypes.c_uint64(0)
                t0 = time.perf_counter()
                rc = lib.mirsha_submit_batch(ctx, arena.ctypes.data, total, off.ctypes.data, lens.ctypes.data, n,
                                             digests.ctypes.data, ctypes.byref(t))
                t1 = time.perf_counter()
                rc = rc or lib.mirsha_wait(ctx, t.value)
                t2 = time.perf_counter()
                assert rc == 0, (name, mode, rc)
                assert np.array_equal(digests, want), (name, mode, it)
                if it >= WARM:
                    ms[mode]["submit"].append((t1 - t0) * 1e3)
                    ms[mode]["wall"].append((t2 - t0) * 1e3)
                    prof[mode].append(eng.host_profile())
        eng.set_order_mode("host")
        out[name] = {"n": n, "bytes": total}
        for mode in ms:
            phases = {k: round(float(np.median([p[k] for p in prof[mode]])), 4)
                      for k in ("validate", "plan", "pack", "device", "scatter")}
            out[name][mode] = {"submit": stats(ms[mode]["submit"]), "wall": stats(ms[mode]["wall"]),
                               "phases_median_ms": phases}
        del arena, digests
    return out


def main():
    import torch

    torch.cuda.is_available()  # torch's HIP runtime first (see tests/conftest.py)
    from mirbft_amd import Engine

    eng = Engine(0)
    line = {"probe": "order_device", "warmup": WARM, "timed": TIMED, "device": torch.cuda.get_device_name(0),
            "host_cpus": len(os.sched_getaffinity(0)), "sort": sort_leg(eng, torch), "cycle": cycle_leg(eng)}
    print(json.dumps(line))
    eng.close()


if __name__ == "__main__":
    main()
