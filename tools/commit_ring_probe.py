#!/usr/bin/env python3
"""The commits' ring form (mirsha_chains_commit_submit) against the synchronous
call: one JSON line.

One process, legs interleaved round by round, 5 warm-up + 30 timed rounds,
medians; the checkpoint values of the legs are compared every round.  The
commit programmes are tools/commit_probe.py's: 64 nodes (chains) commit the same
entries, REPS times 20 batches of 20 request digests and then a checkpoint
(REPS = 1 and 4: 400 writes per node and one checkpoint, 1,600 and four).

(a) "kernel": device time (mirsha_ctx_kernel_time id 1) of the one launch of
    each form: chains_commit_kernel (one lane per chain) and
    chains_commit_seg_kernel (one lane per stretch between checkpoints).
(b) "cycle": one hashing submission (mirsha_submit_batch, page-locked arena and
    output) plus that cycle's commits.  today = mirsha_chains_commit, then
    submit, then wait; ring = commit-submit, submit, wait both.  Wall time per
    cycle and the time until the caller is free (the last submit has
    returned), for 2^20 x 272 B requests (config 2's cycle) and for 1,000.
(c) "priority": the segment kernel's device time alone and beside
    HASH_LAUNCHES back-to-back config-2 request launches (hash_batch_device on
    the engine's stream, device-resident arena), with the waves' issue
    priority 3 and 0 (MIRSHA_AB=1 MIRSHA_COMMIT_PRIO), and the request
    launches' own device time (id 0) in the same rounds.

Usage (GPU box):  python tools/commit_ring_probe.py [--small]
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
NODES, BATCHES, BATCH = 64, 20, 20
REQ_BYTES = 272
HASH_LAUNCHES = 8


def med(v):
    return round(float(np.median(v)), 4)


def stats(v):
    return {"median": med(v), "min": round(float(np.min(v)), 4), "max": round(float(np.max(v)), 4)}


def programme(lib_mod, rng, reps):
    per_cp = BATCHES * BATCH
    table = rng.integers(0, 256, (reps * per_cp, 32), dtype=np.uint8)
    prog = []
    for r in range(reps):
        prog += list(range(r * per_cp, (r + 1) * per_cp)) + [lib_mod.MIRSHA_COMMIT_CHECKPOINT]
    op_digest = np.repeat(np.asarray(prog, dtype=np.uint32), NODES)
    op_chain = np.tile(np.arange(NODES, dtype=np.uint32), len(prog))
    want = []
    for r in range(reps):  # every node's value of checkpoint r
        want += [hashlib.sha256(table[r * per_cp:(r + 1) * per_cp].tobytes()).digest()] * NODES
    return table, op_chain, op_digest, want


def main():
    import torch

    torch.cuda.is_available()  # torch's HIP runtime first (see tests/conftest.py)
    from mirbft_amd import CheckpointChains, Engine, _lib
    from mirbft_amd.engine import KERNEL_LISTS, KERNEL_MSGS

    small = "--small" in sys.argv
    eng = Engine(0)
    rng = np.random.default_rng(1)
    rows = lambda a: [r.tobytes() for r in a]  # noqa: E731
    report = {}

    # ---- (a) device time of the two kernels
    kernel = {}
    for reps in (1, 4):
        table, oc, od, want = programme(_lib, rng, reps)
        sync, ring = CheckpointChains(eng, NODES), CheckpointChains(eng, NODES)
        legs = {"chains_commit_kernel": lambda: sync.commit(table, oc, od),
                "chains_commit_seg_kernel": lambda: eng.wait(ring.submit_commit(table, oc, od))}
        ms = {name: [] for name in legs}
        eng.set_timing(True)
        eng.set_timing_mask([KERNEL_LISTS])
        for it in range(WARM + TIMED):
            for name, call in legs.items():  # interleaved
                eng.reset_timing()
                got = call()
                launches, total = eng.kernel_time(KERNEL_LISTS)
                assert launches == 1 and rows(got) == want, name
                if it >= WARM:
                    ms[name].append(total)
        eng.set_timing(False)
        kernel[f"checkpoints_{reps}"] = {"writes_per_node": reps * BATCHES * BATCH,
                                         "device_ms": {name: stats(v) for name, v in ms.items()}}
        sync.close()
        ring.close()
    report["kernel"] = kernel

    # ---- (b) a hashing submission plus the cycle's commits
    cycle = {}
    for n_req in ((1000,) if small else (1 << 20, 1000)):
        arena = eng.host_empty(n_req * REQ_BYTES)
        tile = rng.integers(0, 256, 1 << 20, dtype=np.uint8)
        for lo in range(0, arena.size, tile.size):
            arena[lo:lo + tile.size] = tile[:min(tile.size, arena.size - lo)]
        arena[:n_req * REQ_BYTES].reshape(n_req, REQ_BYTES)[:, :4] = np.arange(n_req, dtype=np.uint32).view(
            np.uint8).reshape(n_req, 4)  # distinct requests
        off = np.arange(n_req, dtype=np.uint64) * REQ_BYTES
        ln = np.full(n_req, REQ_BYTES, dtype=np.uint32)
        out = eng.host_empty(32 * n_req).reshape(n_req, 32)
        probe_at = [0, n_req // 2, n_req - 1]
        probe_want = [hashlib.sha256(arena[int(off[i]):int(off[i]) + REQ_BYTES].tobytes()).digest() for i in probe_at]
        for reps in (1, 4):
            table, oc, od, want = programme(_lib, rng, reps)
            sync, ring = CheckpointChains(eng, NODES), CheckpointChains(eng, NODES)

            def today():
                t0 = time.perf_counter()
                v = sync.commit(table, oc, od)
                t = eng.submit_batch(arena, off, ln, out=out)
                free = time.perf_counter()
                eng.wait(t)
                return v, (free - t0) * 1e3, (time.perf_counter() - t0) * 1e3

            def on_ring():
                t0 = time.perf_counter()
                tc = ring.submit_commit(table, oc, od)
                t = eng.submit_batch(arena, off, ln, out=out)
                free = time.perf_counter()
                eng.wait(t)  # retires the commit ticket ahead of it
                return tc.values, (free - t0) * 1e3, (time.perf_counter() - t0) * 1e3

            legs = {"today": today, "ring": on_ring}
            free_ms = {name: [] for name in legs}
            wall_ms = {name: [] for name in legs}
            for it in range(WARM + TIMED):
                for name, call in legs.items():  # interleaved
                    out[probe_at] = 0
                    v, free, wall = call()
                    assert rows(v) == want and rows(out[probe_at]) == probe_want, name
                    if it >= WARM:
                        free_ms[name].append(free)
                        wall_ms[name].append(wall)
            cycle[f"requests_{n_req}_checkpoints_{reps}"] = {
                "caller_free_ms": {name: stats(v) for name, v in free_ms.items()},
                "wall_ms": {name: stats(v) for name, v in wall_ms.items()},
            }
            sync.close()
            ring.close()
        del arena, out
    report["cycle"] = cycle

    # ---- (c) the priority of the segment kernel's waves
    n_req = 1000 if small else 1 << 20
    d_arena = torch.randint(0, 256, (n_req * REQ_BYTES + 256,), dtype=torch.uint8, device="cuda")
    d_off = (torch.arange(n_req, dtype=torch.int64, device="cuda") * REQ_BYTES)
    d_len = torch.full((n_req,), REQ_BYTES, dtype=torch.int32, device="cuda")
    d_out = torch.zeros((n_req, 32), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    table, oc, od, want = programme(_lib, rng, 4)
    ring = CheckpointChains(eng, NODES)
    saved = {k: os.environ.get(k) for k in ("MIRSHA_AB", "MIRSHA_COMMIT_PRIO")}
    os.environ["MIRSHA_AB"] = "1"

    def hash_launches():
        for _ in range(HASH_LAUNCHES):
            eng.hash_batch_device(d_arena.data_ptr(), n_req * REQ_BYTES, d_off.data_ptr(), d_len.data_ptr(), None,
                                  n_req, d_out.data_ptr())

    legs = [("alone", 3), ("alone", 0), ("beside", 3), ("beside", 0), ("hash_only", None)]
    commit_ms = {f"{how}_prio{p}": [] for how, p in legs if p is not None}
    hash_ms = {f"{how}_prio{p}" if p is not None else how: [] for how, p in legs if how != "alone"}
    eng.set_timing(True)
    eng.set_timing_mask([KERNEL_MSGS, KERNEL_LISTS])
    for it in range(WARM + TIMED):
        for how, prio in legs:  # interleaved
            name = f"{how}_prio{prio}" if prio is not None else how
            eng.reset_timing()
            if prio is not None:
                os.environ["MIRSHA_COMMIT_PRIO"] = str(prio)
            if how != "alone":
                hash_launches()
            if prio is not None:
                got = eng.wait(ring.submit_commit(table, oc, od))
                assert rows(got) == want, name
            eng.sync()
            if it >= WARM:
                if prio is not None:
                    commit_ms[name].append(eng.kernel_time(KERNEL_LISTS)[1])
                if how != "alone":
                    hash_ms[name].append(eng.kernel_time(KERNEL_MSGS)[1])
    eng.set_timing(False)
    for k, v in saved.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    report["priority"] = {"hash_launches": HASH_LAUNCHES, "requests": n_req, "checkpoints": 4,
                          "commit_device_ms": {k: stats(v) for k, v in commit_ms.items()},
                          "hash_device_ms_sum": {k: stats(v) for k, v in hash_ms.items()}}
    ring.close()
    print(json.dumps({"probe": "commit_ring", "nodes": NODES, "batches": BATCHES, "batch_size": BATCH, "warmup": WARM,
                      "timed": TIMED, "request_bytes": REQ_BYTES, "device": torch.cuda.get_device_name(0), **report}))
    eng.close()


if __name__ == "__main__":
    main()
