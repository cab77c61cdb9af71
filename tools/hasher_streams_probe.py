#!/usr/bin/env python3
"""The streaming hash states under the two hashers: one JSON line.

One process on one MI355X, the legs of a measurement interleaved round by
round, 5 warm-up and 30 timed rounds, medians with min-max; every round's
values are compared with hashlib.

Leg 1: the commit probe's cycle (tools/commit_probe.py): 64 nodes commit the
  same entries, REPS times 20 batches of 20 request digests and then a
  checkpoint (REPS = 1 and 4), through
    stream_log/sha512_256   StreamLog, SHA-512/256 streams
    stream_log/sha256       StreamLog, SHA-256 streams
    device_log/sha512_256   DeviceLog, SHA-512/256 chains
  (a) synchronously (commit_cycle): wall time of the call and the kernel's
      device time from the same call (mirsha_ctx_kernel_time: id 9 for the
      streams, id 1 for the chains);
  (b) as a ring ticket (submit_cycle + collect_cycle): the segment kernel's
      device time, the time until submit_cycle returns (the caller is free) and
      until collect_cycle returns.
  Every cycle ends in a checkpoint, so every round starts from Hasher().
Leg 2: hash.Hash use: 256 hashers, each Write(1 KiB) then Sum(nil), 16 times
  over, all 256 hashers' new bytes and Sums of a step in ONE flush, under both
  hashers: wall time of the 16 flushes and the sum of their kernels' device
  time.

Usage (GPU box):  python tools/hasher_streams_probe.py
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
HASHERS, CHUNK, STEPS = 256, 1024, 16
LEGS = (("stream_log", "sha512_256"), ("stream_log", "sha256"), ("device_log", "sha512_256"))


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
    from mirbft_amd import Checkpoint, Commit, CommitBatch, DeviceLog, Engine, HashStreams, StreamLog
    from mirbft_amd.engine import KERNEL_LISTS, KERNEL_STREAMS

    eng = Engine(0)
    rng = np.random.default_rng(43)
    report = {}
    eng.set_timing(True)
    eng.set_timing_mask([KERNEL_LISTS, KERNEL_STREAMS])
    per_cp = BATCHES * BATCH

    def kernel_ms(kind, launches_want=1):
        launches, ms = eng.kernel_time(KERNEL_STREAMS if kind == "stream_log" else KERNEL_LISTS)
        assert launches == launches_want, (kind, launches)
        return ms

    # ---- leg 1: the commit cycle ---------------------------------------------------------
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
                for h in ("sha256", "sha512_256")}
        logs = {}
        for kind, h in LEGS:
            eng.set_hasher(h)
            logs[kind, h] = (StreamLog if kind == "stream_log" else DeviceLog)(eng, NODES)  # the engine's hasher

        def check(leg, mine, r):
            log, w = logs[leg], want[leg[1]]
            if mine != w or any(log.values[j, node].tobytes() != w[j] for j in range(reps) for node in range(NODES)):
                raise SystemExit(f"{leg}: a checkpoint value differs from hashlib in round {r}")

        def sync_leg(leg):
            def run(r):
                eng.set_hasher(leg[1])
                eng.reset_timing()
                t0 = time.perf_counter()
                mine = logs[leg].commit_cycle(commits)
                wall = (time.perf_counter() - t0) * 1e3
                check(leg, mine, r)
                return {"wall": wall, "kernel": kernel_ms(leg[0])}
            return run

        def ring_leg(leg):
            def run(r):
                eng.set_hasher(leg[1])
                eng.reset_timing()
                t0 = time.perf_counter()
                ticket = logs[leg].submit_cycle(commits)
                free = (time.perf_counter() - t0) * 1e3
                mine = logs[leg].collect_cycle(ticket)
                done = (time.perf_counter() - t0) * 1e3
                check(leg, mine, r)
                return {"caller_free": free, "collected": done, "kernel": kernel_ms(leg[0])}
            return run

        a = rounds({"/".join(leg): sync_leg(leg) for leg in LEGS})
        b = rounds({"/".join(leg): ring_leg(leg) for leg in LEGS})
        report[f"checkpoints_{reps}"] = {"writes_per_node": reps * per_cp, "a_commit_cycle": a, "b_ring_ticket": b}
        for log in logs.values():
            log.close()

    # ---- leg 2: 256 hashers, Write(1 KiB) + Sum, 16 times ---------------------------------
    data = [[rng.bytes(CHUNK) for _ in range(STEPS)] for _ in range(HASHERS)]
    want = {h: [[hashlib.new(h, b"".join(data[k][:step + 1])).digest() for k in range(HASHERS)]
                for step in range(STEPS)] for h in ("sha256", "sha512_256")}
    streams, hashers = {}, {}
    for h in want:
        streams[h] = HashStreams(eng, HASHERS, hasher=h)
        hashers[h] = [streams[h].hasher() for _ in range(HASHERS)]

    def hasher_leg(h):
        def run(r):
            eng.set_hasher(h)
            eng.reset_timing()
            t0 = time.perf_counter()
            out = []
            for x in hashers[h]:
                x.reset()
            for step in range(STEPS):
                for k, x in enumerate(hashers[h]):
                    x.write(data[k][step])
                out.append(streams[h].flush(hashers[h]))
            wall = (time.perf_counter() - t0) * 1e3
            if out != want[h]:
                raise SystemExit(f"{h}: a hasher's sum differs from hashlib in round {r}")
            return {"wall": wall, "kernels": kernel_ms("stream_log", STEPS)}
        return run

    report["hashers"] = {"hashers": HASHERS, "chunk": CHUNK, "steps": STEPS,
                         **rounds({h: hasher_leg(h) for h in want})}
    for s in streams.values():
        s.close()
    eng.set_hasher("sha256")
    eng.set_timing(False)
    print(json.dumps({"probe": "hasher_streams", "device": torch.cuda.get_device_name(0), "nodes": NODES,
                      "batches": BATCHES, "batch_size": BATCH, "warmup_rounds": WARM, "timed_rounds": TIMED,
                      **report}))
    eng.close()


if __name__ == "__main__":
    main()
