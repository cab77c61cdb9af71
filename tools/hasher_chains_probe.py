#!/usr/bin/env python3
"""A cycle's Commits on the device log under the two hashers: one JSON line.

One process on one MI355X, the hashers interleaved round by round (sha256,
sha512_256, sha256, ...), 5 warm-up and 30 timed rounds, medians with
min-max; every round's checkpoint values are compared with hashlib.

The cycle is tools/commit_probe.py's: 64 nodes commit the same entries, REPS
times 20 batches of 20 request digests and then a checkpoint (REPS = 1 and 4).
Every cycle ends in a checkpoint, so every round starts from Hasher() and the
expected values are the same each round.

Leg (a): DeviceLog.commit_cycle (mirsha_chains_commit): wall time of the call
  and the commit kernel's device time (mirsha_ctx_kernel_time id 1), both from
  the same call.
Leg (b): the same cycle as a ring ticket, DeviceLog.submit_cycle +
  collect_cycle: the segment kernel's device time, the time until submit_cycle
  returns (the caller is free) and until collect_cycle returns.  `beside`: the
  same with a 2^20 x 272 B Engine.submit_batch (page-locked arena and rows)
  queued just ahead of the commit ticket, under the same hasher.
Leg (c): without a device log: the application keeps every committed digest
  on the host and calls Engine.digest_lists per checkpoint over the whole list
  (one list per node): wall time per cycle.  The bytes each way sends host to
  device are counted from the shapes.

Usage (GPU box):  python tools/hasher_chains_probe.py
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
HASHERS = ("sha256", "sha512_256")
NODES, BATCHES, BATCH = 64, 20, 20
N, SIZE = 1 << 20, 272


def stats(v):
    return {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(np.min(v)), 4),
            "max_ms": round(float(np.max(v)), 4)}


def rounds(legs):
    """legs: name -> callable(round) -> dict of ms; interleaved, warm-up dropped."""
    got = {k: {} for k in legs}
    for r in range(WARM + TIMED):
        for k, leg in legs.items():
            ms = leg(r)
            if r >= WARM:
                for what, v in ms.items():
                    got[k].setdefault(what, []).append(v)
    return {k: {what: stats(v) for what, v in d.items()} for k, d in got.items()}


def main():
    import torch

    torch.cuda.is_available()  # torch's HIP runtime first (see tests/conftest.py)
    from mirbft_amd import Checkpoint, Commit, CommitBatch, DeviceLog, Engine, commit_plan
    from mirbft_amd.engine import KERNEL_LISTS
    from mirbft_amd.processor import commit_programme

    eng = Engine(0)
    rng = np.random.default_rng(41)
    arena = eng.host_empty(N * SIZE)
    arena[:] = rng.integers(0, 256, size=N * SIZE, dtype=np.uint8)
    off = np.arange(N, dtype=np.uint64) * SIZE
    ln = np.full(N, SIZE, dtype=np.uint32)
    big_rows = eng.host_empty(32 * N).reshape(N, 32)
    spot = [0, N // 2, N - 1]
    big_want = {h: [hashlib.new(h, arena[i * SIZE:(i + 1) * SIZE].tobytes()).digest() for i in spot] for h in HASHERS}
    per_cp = BATCHES * BATCH
    nodes = np.arange(NODES, dtype=np.uint32)
    report = {}
    eng.set_timing(True)
    eng.set_timing_mask([KERNEL_LISTS])
    for reps in (1, 4):
        table = rng.integers(0, 256, (reps * per_cp, 32), dtype=np.uint8)
        commits = []
        for r in range(reps):
            for b in range(BATCHES):
                lo = r * per_cp + b * BATCH
                commits.append(Commit(batch=CommitBatch([table[i].tobytes() for i in range(lo, lo + BATCH)],
                                                        seq_no=r * BATCHES + b + 1)))
            commits.append(Commit(checkpoint=Checkpoint(seq_no=(r + 1) * BATCHES)))
        want = {h: [hashlib.new(h, table[r * per_cp:(r + 1) * per_cp].tobytes()).digest() for r in range(reps)]
                for h in HASHERS}
        logs = {}
        for h in HASHERS:
            eng.set_hasher(h)
            logs[h] = DeviceLog(eng, NODES)  # takes the engine's hasher

        def check(h, log, mine, r):
            if mine != want[h] or any(log.values[j, node].tobytes() != want[h][j]
                                      for j in range(reps) for node in range(NODES)):
                raise SystemExit(f"{h}: a checkpoint value differs from hashlib in round {r}")

        def kernel_ms():
            launches, ms = eng.kernel_time(KERNEL_LISTS)
            assert launches == 1, launches
            return ms

        def sync_leg(h):
            def leg(r):
                eng.set_hasher(h)
                eng.reset_timing()
                t0 = time.perf_counter()
                mine = logs[h].commit_cycle(commits)
                wall = (time.perf_counter() - t0) * 1e3
                check(h, logs[h], mine, r)
                return {"wall": wall, "kernel": kernel_ms()}
            return leg

        def ring_leg(h, beside):
            def leg(r):
                eng.set_hasher(h)
                eng.reset_timing()
                big = None
                t0 = time.perf_counter()
                if beside:
                    big = eng.submit_batch(arena, off, ln, out=big_rows)
                    t0 = time.perf_counter()
                ticket = logs[h].submit_cycle(commits)
                free = (time.perf_counter() - t0) * 1e3
                mine = logs[h].collect_cycle(ticket)
                done = (time.perf_counter() - t0) * 1e3
                out = {"caller_free": free, "collected": done}
                if beside:
                    rows = eng.wait(big)
                    out["hashing_collected"] = (time.perf_counter() - t0) * 1e3
                    if [rows[i].tobytes() for i in spot] != big_want[h]:
                        raise SystemExit(f"{h}: a request digest differs from hashlib in round {r}")
                check(h, logs[h], mine, r)
                out["kernel"] = kernel_ms()
                return out
            return leg

        lists_idx = np.tile(np.arange(per_cp, dtype=np.uint32), NODES)
        lists_first = np.arange(NODES + 1, dtype=np.uint32) * per_cp

        def lists_leg(h):
            def leg(r):
                eng.set_hasher(h)
                t0 = time.perf_counter()
                got = [eng.digest_lists(table[k * per_cp:(k + 1) * per_cp], lists_idx, lists_first) for k in range(reps)]
                wall = (time.perf_counter() - t0) * 1e3
                if any(got[k][node].tobytes() != want[h][k] for k in range(reps) for node in (0, NODES - 1)):
                    raise SystemExit(f"{h}: a list digest differs from hashlib in round {r}")
                return {"wall": wall}
            return leg

        a = rounds({h: sync_leg(h) for h in HASHERS})
        b = rounds({h: ring_leg(h, False) for h in HASHERS})
        b2 = rounds({h: ring_leg(h, True) for h in HASHERS})
        c = rounds({h: lists_leg(h) for h in HASHERS})
        op_table, op_chain, op_digest = commit_programme(commits, NODES)
        _, _, ent, _ = commit_plan(op_chain, op_digest, NODES, op_table.shape[0])
        h2d = {"device_log_commit": 32 * op_table.shape[0] + 4 * (2 * NODES + 1 + ent.size),
               "digest_lists_per_checkpoint": reps * (32 * per_cp + 4 * lists_idx.size + 4 * lists_first.size)}
        report[f"checkpoints_{reps}"] = {"writes_per_node": reps * per_cp, "a_commit_cycle": a, "b_ring_ticket": b,
                                         "b_ring_ticket_beside_submit_batch": b2, "c_digest_lists_per_checkpoint": c,
                                         "h2d_bytes": h2d}
        for log in logs.values():
            log.close()
    eng.set_timing(False)
    print(json.dumps({"probe": "hasher_chains", "device": torch.cuda.get_device_name(0), "nodes": NODES,
                      "batches": BATCHES, "batch_size": BATCH, "warmup_rounds": WARM, "timed_rounds": TIMED,
                      "beside": {"n": N, "request_bytes": SIZE}, **report}))
    eng.close()


if __name__ == "__main__":
    main()
