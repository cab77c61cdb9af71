#!/usr/bin/env python3
"""The streams' ring form (mirsha_streams_submit) against the synchronous call:
one JSON line.

One process, legs interleaved round by round, 5 warm-up + 30 timed rounds,
median (min-max); every round's values are compared with hashlib.  The
programmes are tools/commit_ring_probe.py's, as a StreamLog writes them: 64
nodes (streams) apply the same entries, REPS times 20 batches of 20 request
digests (one 640-byte write per batch and node, every node naming the same
range) and then a Sum-then-Reset (REPS = 1 and 4).

(a) "kernel": device time (mirsha_ctx_kernel_time id 9) of the one launch of
    each form: streams_kernel (one lane per stream) and streams_seg_kernel (one
    lane per stretch between resets).
(b) "cycle": one hashing submission (mirsha_submit_batch, page-locked arena and
    output) plus that cycle's stream programme.  today = mirsha_streams_run,
    then submit, then wait; ring = streams-submit, submit, wait both.  Wall
    time per cycle and the time until the caller is free (the last submit has
    returned), for 2^20 x 272 B requests (config 2's cycle) and for 1,000.
(c) "logs": StreamLog.submit_cycle / collect_cycle against DeviceLog's on the
    same commits: the time until submit_cycle has returned, and until
    collect_cycle has.

Usage (GPU box):  python tools/streams_ring_probe.py [--small]
"""
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


def stats(v):
    return {"median": round(float(np.median(v)), 4), "min": round(float(np.min(v)), 4),
            "max": round(float(np.max(v)), 4)}


def programme(lib_mod, rng, reps):
    """(ops, arena, want): the stream programme and every node's value of each checkpoint."""
    per_cp = BATCHES * BATCH * 32
    arena = rng.integers(0, 256, reps * per_cp, dtype=np.uint8)
    kinds, offs, lens = [], [], []
    for r in range(reps):
        for b in range(BATCHES):
            kinds.append(lib_mod.MIRSHA_STREAM_WRITE)
            offs.append(r * per_cp + b * BATCH * 32)
            lens.append(BATCH * 32)
        kinds.append(lib_mod.MIRSHA_STREAM_SUM_RESET)
        offs.append(0)
        lens.append(0)
    ops = (np.tile(np.arange(NODES, dtype=np.uint32), len(kinds)), np.repeat(np.asarray(kinds, dtype=np.uint32), NODES),
           np.repeat(np.asarray(offs, dtype=np.uint64), NODES), np.repeat(np.asarray(lens, dtype=np.uint32), NODES))
    want = []
    for r in range(reps):
        want += [hashlib.sha256(arena[r * per_cp:(r + 1) * per_cp].tobytes()).digest()] * NODES
    return ops, arena, want


def commits_of(rng, reps):
    """The same shape as Commit objects, for the two logs; (commits, want per checkpoint)."""
    from mirbft_amd import Checkpoint, Commit, CommitBatch

    commits, want, seq = [], [], 0
    for r in range(reps):
        h = hashlib.sha256()
        for _ in range(BATCHES):
            seq += 1
            digests = [rng.bytes(32) for _ in range(BATCH)]
            h.update(b"".join(digests))
            commits.append(Commit(batch=CommitBatch(digests, seq_no=seq)))
        commits.append(Commit(checkpoint=Checkpoint(seq_no=seq)))
        want.append(h.digest())
    return commits, want


def main():
    import torch

    torch.cuda.is_available()  # torch's HIP runtime first (see tests/conftest.py)
    from mirbft_amd import DeviceLog, Engine, HashStreams, StreamLog, _lib
    from mirbft_amd.engine import KERNEL_STREAMS

    small = "--small" in sys.argv
    eng = Engine(0)
    rng = np.random.default_rng(1)
    rows = lambda a: [r.tobytes() for r in a]  # noqa: E731
    report = {}

    # ---- (a) device time of the two kernels
    kernel = {}
    for reps in (1, 4):
        ops, sarena, want = programme(_lib, rng, reps)
        sync, ring = HashStreams(eng, NODES), HashStreams(eng, NODES)
        legs = {"streams_kernel": lambda: sync.run(ops, sarena),
                "streams_seg_kernel": lambda: eng.wait(ring.submit(ops, sarena))}
        ms = {name: [] for name in legs}
        eng.set_timing(True)
        eng.set_timing_mask([KERNEL_STREAMS])
        for it in range(WARM + TIMED):
            for name, call in legs.items():  # interleaved
                eng.reset_timing()
                got = call()
                launches, total = eng.kernel_time(KERNEL_STREAMS)
                assert launches == 1 and rows(got) == want, name
                if it >= WARM:
                    ms[name].append(total)
        eng.set_timing(False)
        kernel[f"checkpoints_{reps}"] = {"bytes_per_node": reps * BATCHES * BATCH * 32,
                                         "device_ms": {name: stats(v) for name, v in ms.items()}}
        sync.close()
        ring.close()
    report["kernel"] = kernel

    # ---- (b) a hashing submission plus the cycle's stream programme
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
            ops, sarena, want = programme(_lib, rng, reps)
            sync, ring = HashStreams(eng, NODES), HashStreams(eng, NODES)

            def today():
                t0 = time.perf_counter()
                v = sync.run(ops, sarena)
                t = eng.submit_batch(arena, off, ln, out=out)
                free = time.perf_counter()
                eng.wait(t)
                return v, (free - t0) * 1e3, (time.perf_counter() - t0) * 1e3

            def on_ring():
                t0 = time.perf_counter()
                ts = ring.submit(ops, sarena)
                t = eng.submit_batch(arena, off, ln, out=out)
                free = time.perf_counter()
                eng.wait(t)  # retires the stream ticket ahead of it
                return ts.values, (free - t0) * 1e3, (time.perf_counter() - t0) * 1e3

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

    # ---- (c) the two logs' asynchronous form
    logs = {}
    for reps in (1, 4):
        commits, want = commits_of(rng, reps)
        made = {"StreamLog": StreamLog(eng, NODES), "DeviceLog": DeviceLog(eng, NODES)}
        queued_ms = {name: [] for name in made}
        wall_ms = {name: [] for name in made}
        for it in range(WARM + TIMED):
            for name, log in made.items():  # interleaved
                t0 = time.perf_counter()
                ticket = log.submit_cycle(commits)
                queued = time.perf_counter()
                got = log.collect_cycle(ticket)
                wall = time.perf_counter()
                assert got == want and all(rows(log.values[:, k]) == want for k in range(NODES)), name
                if it >= WARM:
                    queued_ms[name].append((queued - t0) * 1e3)
                    wall_ms[name].append((wall - t0) * 1e3)
        logs[f"checkpoints_{reps}"] = {"submit_cycle_ms": {name: stats(v) for name, v in queued_ms.items()},
                                       "submit_and_collect_ms": {name: stats(v) for name, v in wall_ms.items()}}
        for log in made.values():
            log.close()
    report["logs"] = logs

    print(json.dumps({"probe": "streams_ring", "nodes": NODES, "batches": BATCHES, "batch_size": BATCH, "warmup": WARM,
                      "timed": TIMED, "request_bytes": REQ_BYTES, "device": torch.cuda.get_device_name(0), **report}))
    eng.close()


if __name__ == "__main__":
    main()
