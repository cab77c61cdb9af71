#!/usr/bin/env python3
"""One commit call vs the write / sum / reset calls for the same cycle: one JSON line.

The cycle: 64 nodes (chains) commit the same entries, REPS times 20 batches of
20 request digests and then a checkpoint (testengine: NodeState.Commit on every
node, testengine/recorder.go:213-256).  One-call form: mirsha_chains_commit
with the digest table passed once.  Three-call form: per checkpoint one
mirsha_chains_absorb (every node's copy of every digest uploaded),
mirsha_chains_sum and mirsha_chains_reset.  Both straight through the C-ABI
from arrays built beforehand, interleaved A/B in one process on two
mirsha_chains objects: 5 warm-up and 30 timed cycles each, medians of a host
clock around the synchronous calls; the values of the two forms are compared
every cycle.  Then the device time of the launches (mirsha_ctx_kernel_time id
1) of one cycle of each form, and the bytes each form copies host to device,
counted from the shapes.

Usage (GPU box):  python tools/commit_probe.py
"""
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

WARM, TIMED = 5, 30
NODES, BATCHES, BATCH = 64, 20, 20


def main():
    import torch

    torch.cuda.is_available()  # torch's HIP runtime first (see tests/conftest.py)
    from mirbft_amd import CheckpointChains, Engine, _lib, commit_plan
    from mirbft_amd.engine import KERNEL_LISTS

    eng = Engine(0)
    lib, ctx = eng._lib, eng.ctx
    p = lambda a: a.ctypes.data  # noqa: E731
    rng = np.random.default_rng(1)
    per_cp = BATCHES * BATCH
    nodes = np.arange(NODES, dtype=np.uint32)
    report = {}
    for reps in (1, 4):
        table = rng.integers(0, 256, (reps * per_cp, 32), dtype=np.uint8)
        prog = []
        for r in range(reps):
            prog += list(range(r * per_cp, (r + 1) * per_cp)) + [_lib.MIRSHA_COMMIT_CHECKPOINT]
        op_digest = np.repeat(np.asarray(prog, dtype=np.uint32), NODES)
        op_chain = np.tile(nodes, len(prog))
        values = np.zeros((reps * NODES, 32), dtype=np.uint8)
        k = ctypes.c_uint32(0)
        # three-call form: each node's copy of each digest, in write order
        absorb_d = [np.ascontiguousarray(np.repeat(table[r * per_cp:(r + 1) * per_cp], NODES, axis=0))
                    for r in range(reps)]
        absorb_c = np.tile(nodes, per_cp)
        sums = np.zeros((reps, NODES, 32), dtype=np.uint8)
        one, three = CheckpointChains(eng, NODES), CheckpointChains(eng, NODES)

        def one_call():
            rc = lib.mirsha_chains_commit(ctx, one.handle, p(table), table.shape[0], p(op_chain), p(op_digest),
                                          op_chain.size, p(values), ctypes.byref(k))
            assert rc == 0 and k.value == reps * NODES, rc

        def three_calls():
            for r in range(reps):
                rc = lib.mirsha_chains_absorb(ctx, three.handle, p(absorb_d[r]), p(absorb_c), absorb_c.size)
                rc |= lib.mirsha_chains_sum(ctx, three.handle, p(nodes), NODES, p(sums[r]))
                rc |= lib.mirsha_chains_reset(ctx, three.handle, p(nodes), NODES)
                assert rc == 0, rc

        legs = {"one_call": one_call, "three_calls": three_calls}
        ms = {name: [] for name in legs}
        for it in range(WARM + TIMED):
            for name, call in legs.items():  # interleaved
                t0 = time.perf_counter()
                call()
                dt = (time.perf_counter() - t0) * 1e3
                if it >= WARM:
                    ms[name].append(dt)
            assert np.array_equal(values.reshape(reps, NODES, 32), sums)
        kern = {}
        eng.set_timing(True)
        eng.set_timing_mask([KERNEL_LISTS])
        for name, call in legs.items():
            eng.reset_timing()
            call()
            launches, total = eng.kernel_time(KERNEL_LISTS)
            kern[name] = {"launches": int(launches), "device_ms": round(float(total), 4)}
        eng.set_timing(False)
        act, efirst, ent, _ = commit_plan(op_chain, op_digest, NODES, table.shape[0])
        cap = min(op_chain.size, NODES)
        h2d = {"one_call": 32 * table.shape[0] + 4 * (2 * cap + 1 + ent.size),
               "three_calls": reps * (32 * absorb_c.size + 4 * absorb_c.size + 4 * NODES + 4 * (NODES + 1)
                                      + 4 * NODES + 4 * NODES)}
        report[f"checkpoints_{reps}"] = {
            "writes_per_node": reps * per_cp,
            "host_ms": {name: {"median": round(float(np.median(v)), 4), "min": round(float(np.min(v)), 4)}
                        for name, v in ms.items()},
            "one_over_three": round(float(np.median(ms["one_call"]) / np.median(ms["three_calls"])), 4),
            "kernels": kern, "h2d_bytes": h2d,
        }
        one.close()
        three.close()
    print(json.dumps({"probe": "commit", "nodes": NODES, "batches": BATCHES, "batch_size": BATCH, "warmup": WARM,
                      "timed": TIMED, "device": torch.cuda.get_device_name(0), **report}))
    eng.close()


if __name__ == "__main__":
    main()
