#!/usr/bin/env python3
"""The SHA-512/256 chains' commit launches, one-lane against pair: one JSON line.

One process on one MI355X.  The one-lane kernels' source is what it was, so the
two legs are Engine.set_variant(5) (the one-lane kernel at any size) and
set_variant(6) (the pair kernel at any size) on two chains objects of ONE
context, interleaved round by round (one_lane, pair, one_lane, ...), 5 warm-up
and 30 timed rounds, medians with min-max.  Every round's checkpoint values and
the chains' final sums are compared with the other leg's, the first round's
with hashlib as well, and every call's route is asserted by the change of
CheckpointChains.pair_launches.

(a) DeviceLog.commit_cycle (mirsha_chains_commit) of tools/hasher_chains_probe.py's
    cycle: 64 nodes commit the same entries, REPS times 20 batches of 20 request
    digests and then a checkpoint (REPS = 1 and 4): the commit kernel's device
    time (mirsha_ctx_kernel_time id 1) and the call's wall time.
(b) The same cycle as a ring ticket (submit_cycle + collect_cycle): the segment
    kernel's device time, the time until the caller is free and until the
    values are collected; alone, and beside a 2^20 x 272 B Engine.submit_batch
    queued just ahead of it.
(c) 1, 2, 64, 256 and 384 groups of 64 chains with 40 writes and a checkpoint
    each, CheckpointChains.commit: device time and wall time.  `pair_wins`: the
    pair's median lies below the one-lane leg's minimum (the rule that set
    kSha512PairMaxGroups).

Usage (GPU box):  python tools/hasher_chains_pair_probe.py
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
LEGS = {"one_lane": 5, "pair": 6}
NODES, BATCHES, BATCH = 64, 20, 20
N, SIZE = 1 << 20, 272
GROUPS, WRITES = (1, 2, 64, 256, 384), 40


def stats(v):
    return {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(np.min(v)), 4),
            "max_ms": round(float(np.max(v)), 4)}


def rounds(leg, same):
    """leg(name, round) -> (dict of ms, what the round computed); the legs
    interleaved, warm-up dropped; same(a, b, round) compares what two legs computed."""
    got = {k: {} for k in LEGS}
    for r in range(WARM + TIMED):
        results = {}
        for k in LEGS:
            ms, results[k] = leg(k, r)
            if r >= WARM:
                for what, v in ms.items():
                    got[k].setdefault(what, []).append(v)
        same(results["one_lane"], results["pair"], r)
    out = {k: {what: stats(v) for what, v in d.items()} for k, d in got.items()}
    out["pair_wins"] = out["pair"]["kernel"]["median_ms"] < out["one_lane"]["kernel"]["min_ms"]
    out["pair_over_one_lane"] = round(out["pair"]["kernel"]["median_ms"] / out["one_lane"]["kernel"]["median_ms"], 3)
    return out


def main():
    import torch

    torch.cuda.is_available()  # torch's HIP runtime first (see tests/conftest.py)
    from mirbft_amd import (Checkpoint, CheckpointChains, Commit, CommitBatch, DeviceLog, Engine, _lib,
                            sha512_pair_max_groups)
    from mirbft_amd.engine import KERNEL_LISTS

    CP = _lib.MIRSHA_COMMIT_CHECKPOINT
    H = lambda b: hashlib.new("sha512_256", b).digest()
    eng = Engine(0)
    eng.set_hasher("sha512_256")
    rng = np.random.default_rng(43)
    arena = eng.host_empty(N * SIZE)
    arena[:] = rng.integers(0, 256, size=N * SIZE, dtype=np.uint8)
    off = np.arange(N, dtype=np.uint64) * SIZE
    ln = np.full(N, SIZE, dtype=np.uint32)
    big_rows = eng.host_empty(32 * N).reshape(N, 32)
    spot = [0, N // 2, N - 1]
    big_want = [H(arena[i * SIZE:(i + 1) * SIZE].tobytes()) for i in spot]
    per_cp = BATCHES * BATCH
    report = {}
    eng.set_timing(True)
    eng.set_timing_mask([KERNEL_LISTS])

    def kernel_ms():
        launches, ms = eng.kernel_time(KERNEL_LISTS)
        assert launches == 1, launches
        return ms

    def routed(chains, name, before):
        took = chains.pair_launches - before
        if took != (1 if name == "pair" else 0):
            raise SystemExit(f"{name}: {took} pair launches in one call")

    def same(a, b, r):
        if a != b:
            raise SystemExit(f"the legs' values or sums differ in round {r}")

    for reps in (1, 4):
        table = rng.integers(0, 256, (reps * per_cp, 32), dtype=np.uint8)
        commits = []
        for k in range(reps):
            for b in range(BATCHES):
                lo = k * per_cp + b * BATCH
                commits.append(Commit(batch=CommitBatch([table[i].tobytes() for i in range(lo, lo + BATCH)],
                                                        seq_no=k * BATCHES + b + 1)))
            commits.append(Commit(checkpoint=Checkpoint(seq_no=(k + 1) * BATCHES)))
        want = [H(table[k * per_cp:(k + 1) * per_cp].tobytes()) for k in range(reps)]
        logs = {name: DeviceLog(eng, NODES) for name in LEGS}

        def computed(name, mine, r):
            log = logs[name]
            vals = [log.values[j, node].tobytes() for j in range(reps) for node in range(NODES)]
            final = [g.tobytes() for g in log.chains.sum(np.arange(NODES, dtype=np.uint32))]
            if r == 0 and (mine != want or vals != [w for w in want for _ in range(NODES)]):
                raise SystemExit(f"{name}: a checkpoint value differs from hashlib")
            return mine, vals, final

        def sync_leg(name, r):
            eng.set_variant(LEGS[name])
            eng.reset_timing()
            before = logs[name].chains.pair_launches
            t0 = time.perf_counter()
            mine = logs[name].commit_cycle(commits)
            wall = (time.perf_counter() - t0) * 1e3
            ms = {"kernel": kernel_ms(), "wall": wall}
            routed(logs[name].chains, name, before)
            return ms, computed(name, mine, r)

        def ring_leg(beside):
            def leg(name, r):
                eng.reset_timing()
                before = logs[name].chains.pair_launches
                big = None
                if beside:  # the hashing takes the automatic route in both legs (timing id 0: masked out)
                    eng.set_variant(0)
                    big = eng.submit_batch(arena, off, ln, out=big_rows)
                eng.set_variant(LEGS[name])  # read when the ticket is queued
                t0 = time.perf_counter()
                ticket = logs[name].submit_cycle(commits)
                free = (time.perf_counter() - t0) * 1e3
                mine = logs[name].collect_cycle(ticket)
                ms = {"caller_free": free, "collected": (time.perf_counter() - t0) * 1e3}
                if beside:
                    rows = eng.wait(big)
                    if [rows[i].tobytes() for i in spot] != big_want:
                        raise SystemExit(f"{name}: a request digest differs from hashlib in round {r}")
                ms["kernel"] = kernel_ms()
                routed(logs[name].chains, name, before)
                return ms, computed(name, mine, r)
            return leg

        report[f"checkpoints_{reps}"] = {"writes_per_node": reps * per_cp, "a_commit_cycle": rounds(sync_leg, same),
                                         "b_ring_ticket": rounds(ring_leg(False), same),
                                         "b_ring_ticket_beside_submit_batch": rounds(ring_leg(True), same)}
        for log in logs.values():
            log.close()

    sweep = {}
    table = rng.integers(0, 256, (64, 32), dtype=np.uint8)
    for groups in GROUPS:
        n = 64 * groups
        # chain c writes rows (c + i) % 64, i = 0..39, then takes its checkpoint; chain-major op order
        oc = np.repeat(np.arange(n, dtype=np.uint32), WRITES + 1)
        od = np.empty((n, WRITES + 1), dtype=np.uint32)
        od[:, :WRITES] = (np.arange(n, dtype=np.uint32)[:, None] + np.arange(WRITES, dtype=np.uint32)[None, :]) % 64
        od[:, WRITES] = CP
        od = od.reshape(-1)
        want64 = [H(b"".join(table[(c + i) % 64].tobytes() for i in range(WRITES))) for c in range(64)]
        chains = {name: CheckpointChains(eng, n) for name in LEGS}
        probe_ids = np.asarray([0, n // 2, n - 1], dtype=np.uint32)

        def sweep_leg(name, r):
            eng.set_variant(LEGS[name])
            eng.reset_timing()
            before = chains[name].pair_launches
            t0 = time.perf_counter()
            got = chains[name].commit(table, oc, od)
            wall = (time.perf_counter() - t0) * 1e3
            ms = {"kernel": kernel_ms(), "wall": wall}
            routed(chains[name], name, before)
            if r == 0 and any(got[c].tobytes() != want64[c % 64] for c in range(n)):
                raise SystemExit(f"{name}: a checkpoint value differs from hashlib ({groups} groups)")
            return ms, (got.tobytes(), chains[name].sum(probe_ids).tobytes())

        sweep[str(groups)] = rounds(sweep_leg, same)
        for ch in chains.values():
            ch.close()
    report["c_groups_of_40_writes_and_a_checkpoint"] = sweep
    wins = [g for g in GROUPS if sweep[str(g)]["pair_wins"]]
    report["largest_group_count_where_the_pair_wins"] = max(wins) if wins else 0
    eng.set_timing(False)
    eng.set_variant(0)
    print(json.dumps({"probe": "hasher_chains_pair", "device": torch.cuda.get_device_name(0), "nodes": NODES,
                      "batches": BATCHES, "batch_size": BATCH, "warmup_rounds": WARM, "timed_rounds": TIMED,
                      "legs": LEGS, "threshold_in_force": sha512_pair_max_groups(),
                      "beside": {"n": N, "request_bytes": SIZE}, **report}))
    eng.close()


if __name__ == "__main__":
    main()
