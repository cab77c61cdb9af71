#!/usr/bin/env python3
"""The streaming hash states against what they stand beside: one JSON line.

(a) hash.Hash use: 256 hashers, each Write(1 KiB) then Sum(nil), 16 times over
    (every hasher ends at 16 KiB).  today = ``GpuHash``: the bytes stay on the
    host and every Sum re-hashes the whole message in a call of its own.
    streams = ``HashStreams.hasher()``: per step all 256 hashers' new bytes
    and Sums go in ONE ``flush``, the states stay on the device.
(b) the commit probe's cycle (tools/commit_probe.py): 64 nodes commit the
    same 20 batches of 20 request digests, then a checkpoint, through
    ``StreamLog.commit_cycle`` and through ``DeviceLog.commit_cycle``.

One process on one device, the two legs of a measurement interleaved round by
round, 5 warm-up and 30 timed rounds, a host clock around the synchronous
calls; every round's values are checked (hashlib for (a), leg against leg and
hashlib for (b)).  Then the device time of one round of each leg
(mirsha_ctx_kernel_time) and the bytes each leg sends host to device.

Usage (GPU box):  python tools/streams_probe.py
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
HASHERS, CHUNK, STEPS = 256, 1024, 16
NODES, BATCHES, BATCH = 64, 20, 20


def stats(v):
    return {"median": round(float(np.median(v)), 4), "min": round(float(np.min(v)), 4),
            "max": round(float(np.max(v)), 4)}


def interleaved(legs, check):
    ms = {name: [] for name in legs}
    for it in range(WARM + TIMED):
        got = {}
        for name, call in legs.items():
            t0 = time.perf_counter()
            got[name] = call()
            dt = (time.perf_counter() - t0) * 1e3
            if it >= WARM:
                ms[name].append(dt)
        check(got)
    return ms


def device_time(eng, legs, kernels):
    out = {}
    eng.set_timing(True)
    eng.set_timing_mask(kernels)
    for name, call in legs.items():
        eng.reset_timing()
        call()
        per = {k: eng.kernel_time(k) for k in kernels}
        out[name] = {"launches": int(sum(n for n, _ in per.values())),
                     "device_ms": round(float(sum(t for _, t in per.values())), 4)}
    eng.set_timing(False)
    eng.set_timing_mask(range(32))
    return out


def main():
    import torch

    torch.cuda.is_available()  # torch's HIP runtime first (see tests/conftest.py)
    from mirbft_amd import (Checkpoint, Commit, CommitBatch, DeviceLog, Engine, GpuHash, HashStreams, StreamLog)
    from mirbft_amd.engine import KERNEL_LISTS, KERNEL_MSGS, KERNEL_STREAMS

    eng = Engine(0)
    rng = np.random.default_rng(1)
    report = {}

    # ---- (a) 256 hashers, Write(1 KiB) + Sum, 16 times -----------------------------------
    data = [[rng.bytes(CHUNK) for _ in range(STEPS)] for _ in range(HASHERS)]
    want = []
    for step in range(STEPS):
        want.append([hashlib.sha256(b"".join(data[h][:step + 1])).digest() for h in range(HASHERS)])
    old = [GpuHash(eng) for _ in range(HASHERS)]
    hs = HashStreams(eng, HASHERS)
    new = [hs.hasher() for _ in range(HASHERS)]

    def today():
        out = []
        for h in old:
            h.reset()
        for step in range(STEPS):
            row = []
            for k, h in enumerate(old):
                h.write(data[k][step])
                row.append(h.sum())
            out.append(row)
        return out

    def streams():
        out = []
        for h in new:
            h.reset()
        for step in range(STEPS):
            for k, h in enumerate(new):
                h.write(data[k][step])
            out.append(hs.flush(new))
        return out

    def check_a(got):
        assert got["gpuhash"] == want and got["streams"] == want

    legs = {"gpuhash": today, "streams": streams}
    ms = interleaved(legs, check_a)
    sent0 = hs.bytes_sent
    streams()
    sent = hs.bytes_sent - sent0
    report["hashers"] = {
        "hashers": HASHERS, "chunk": CHUNK, "steps": STEPS,
        "host_ms": {k: stats(v) for k, v in ms.items()},
        "streams_over_gpuhash": round(float(np.median(ms["streams"]) / np.median(ms["gpuhash"])), 4),
        "kernels": device_time(eng, legs, [KERNEL_MSGS, KERNEL_STREAMS]),
        "h2d_message_bytes": {"gpuhash": HASHERS * CHUNK * STEPS * (STEPS + 1) // 2,
                              "streams": sent},
    }
    hs.close()

    # ---- (b) the commit probe's cycle --------------------------------------------------------
    commits = [Commit(batch=CommitBatch(digests=[rng.bytes(32) for _ in range(BATCH)], seq_no=s + 1))
               for s in range(BATCHES)] + [Commit(checkpoint=Checkpoint(seq_no=BATCHES))]
    value = hashlib.sha256(b"".join(d for c in commits[:-1] for d in c.batch.digests)).digest()
    slog, dlog = StreamLog(eng, NODES), DeviceLog(eng, NODES)

    def check_b(got):
        assert got["stream_log"] == got["device_log"] == [value]
        assert np.array_equal(slog.values, dlog.values) and slog.values.shape == (1, NODES, 32)

    legs = {"stream_log": lambda: slog.commit_cycle(commits), "device_log": lambda: dlog.commit_cycle(commits)}
    ms = interleaved(legs, check_b)
    sent0 = slog.streams.bytes_sent
    slog.commit_cycle(commits)
    sent = slog.streams.bytes_sent - sent0
    report["commit_cycle"] = {
        "nodes": NODES, "batches": BATCHES, "batch_size": BATCH,
        "host_ms": {k: stats(v) for k, v in ms.items()},
        "stream_over_device_log": round(float(np.median(ms["stream_log"]) / np.median(ms["device_log"])), 4),
        "kernels": device_time(eng, legs, [KERNEL_LISTS, KERNEL_STREAMS]),
        "h2d_message_bytes": {"stream_log": sent, "device_log": 32 * BATCHES * BATCH},
    }
    slog.close()
    dlog.close()
    print(json.dumps({"probe": "streams", "warmup": WARM, "timed": TIMED, "device": torch.cuda.get_device_name(0),
                      **report}))
    eng.close()


if __name__ == "__main__":
    main()
