#!/usr/bin/env python3
"""The two hashers of a context side by side: one JSON line.

One process on one MI355X, the hashers interleaved round by round (sha256,
sha512_256, sha256, ...), 5 warm-up and 30 timed rounds, medians with
min-max; every round's digests are spot-checked against hashlib.

Leg (a): the config-2 shape, 2^20 requests of 272 B already on the device,
  mirsha_hash_batch_device: the request kernel's device time
  (mirsha_ctx_kernel_time id 0), digests/s and compressions/s (5 per message
  for SHA-256, 3 for SHA-512/256).
Leg (b): the same cycle from the host: mirsha_hash_batch from a page-locked
  arena (wall time of the call), and mirsha_submit_batch into page-locked rows
  (submit to mirsha_wait returning).
Leg (c): batches of 20 over those 2^20 digests, mirsha_digest_lists_device:
  the list kernel's device time (id 1).

Usage (GPU box):  python tools/hasher_probe.py
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
N, SIZE, BATCH = 1 << 20, 272, 20
COMPRESSIONS = {"sha256": (SIZE + 72) // 64, "sha512_256": (SIZE + 16) // 128 + 1}
LIST_COMPRESSIONS = {"sha256": (32 * BATCH + 72) // 64, "sha512_256": (32 * BATCH + 16) // 128 + 1}


def stats(v):
    return {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(np.min(v)), 4),
            "max_ms": round(float(np.max(v)), 4)}


def oracle(name, b):
    return hashlib.new(name, bytes(b)).digest()


def rounds(legs):
    """legs: name -> callable(round) -> ms; interleaved, warm-up dropped."""
    got = {k: [] for k in legs}
    for r in range(WARM + TIMED):
        for k, leg in legs.items():
            ms = leg(r)
            if r >= WARM:
                got[k].append(ms)
    return got


def main():
    import torch

    assert torch.cuda.is_available()
    from mirbft_amd import Engine, sharding
    from mirbft_amd.engine import KERNEL_LISTS, KERNEL_MSGS

    eng = Engine(0)
    rng = np.random.default_rng(31)
    arena = eng.host_empty(N * SIZE)
    arena[:] = rng.integers(0, 256, size=N * SIZE, dtype=np.uint8)
    off = np.arange(N, dtype=np.uint64) * SIZE
    ln = np.full(N, SIZE, dtype=np.uint32)
    spots = rng.integers(0, N, size=(WARM + TIMED, 4))
    want = {h: {int(i): oracle(h, arena[i * SIZE:(i + 1) * SIZE]) for i in np.unique(spots)} for h in HASHERS}

    def check(h, got_rows, r):
        for i in spots[r]:
            if bytes(got_rows[int(i)]) != want[h][int(i)]:
                raise SystemExit(f"{h}: digest {int(i)} differs from hashlib in round {r}")

    d_arena = torch.from_numpy(np.asarray(arena)).cuda()
    d_off, d_len = torch.from_numpy(off.view(np.int64)).cuda(), torch.from_numpy(ln.view(np.int32)).cuda()
    d_out = {h: torch.empty((N, 32), dtype=torch.uint8, device="cuda") for h in HASHERS}
    idx, first = sharding.batch_lists(N, BATCH)
    n_lists = int(first.size) - 1
    d_idx, d_first = torch.from_numpy(idx.view(np.int32)).cuda(), torch.from_numpy(first.view(np.int32)).cuda()
    d_lists = torch.empty((n_lists, 32), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    eng.set_timing(True)

    def kernel_leg(h, kernel, launch, verify):
        def leg(r):
            eng.set_hasher(h)
            eng.reset_timing()
            launch(h)
            eng.sync()
            launches, ms = eng.kernel_time(kernel)
            assert launches == 1, launches
            verify(h, r)
            return ms
        return leg

    def launch_msgs(h):
        eng.hash_batch_device(d_arena.data_ptr(), N * SIZE, d_off.data_ptr(), d_len.data_ptr(), None, N,
                              d_out[h].data_ptr())

    def verify_msgs(h, r):
        rows = d_out[h][torch.from_numpy(spots[r])].cpu().numpy()
        check(h, {int(i): rows[k] for k, i in enumerate(spots[r])}, r)

    a = rounds({h: kernel_leg(h, KERNEL_MSGS, launch_msgs, verify_msgs) for h in HASHERS})

    list_want = {}

    def launch_lists(h):
        eng.digest_lists_device(d_out[h].data_ptr(), N, d_idx.data_ptr(), d_first.data_ptr(), n_lists, int(idx.size),
                                d_lists.data_ptr())

    def verify_lists(h, r):
        b = int(spots[r][0]) % n_lists
        if (h, b) not in list_want:
            members = d_out[h][b * BATCH: min((b + 1) * BATCH, N)].cpu().numpy().tobytes()
            list_want[(h, b)] = oracle(h, members)
        if d_lists[b].cpu().numpy().tobytes() != list_want[(h, b)]:
            raise SystemExit(f"{h}: list digest {b} differs from hashlib in round {r}")

    c = rounds({h: kernel_leg(h, KERNEL_LISTS, launch_lists, verify_lists) for h in HASHERS})
    eng.set_timing(False)

    out_rows = eng.host_empty(32 * N).reshape(N, 32)

    def host_leg(h, call):
        def leg(r):
            eng.set_hasher(h)
            t0 = time.perf_counter()
            rows = call()
            ms = (time.perf_counter() - t0) * 1e3
            check(h, rows, r)
            return ms
        return leg

    sync_out = np.empty((N, 32), dtype=np.uint8)
    b_sync = rounds({h: host_leg(h, lambda: eng.hash_batch(arena, off, ln, out=sync_out)) for h in HASHERS})
    b_ring = rounds({h: host_leg(h, lambda: eng.wait(eng.submit_batch(arena, off, ln, out=out_rows))) for h in HASHERS})
    eng.close()

    res = {"device": torch.cuda.get_device_name(0), "n": N, "request_bytes": SIZE, "batch": BATCH, "n_lists": n_lists,
           "warmup_rounds": WARM, "timed_rounds": TIMED, "a_hash_batch_device": {}, "b_hash_batch_pinned": {},
           "b_submit_batch_pinned_rows": {}, "c_digest_lists_device": {}}
    for h in HASHERS:
        s = stats(a[h])
        s["digests_per_s"] = round(N / (s["median_ms"] * 1e-3))
        s["compressions_per_message"] = COMPRESSIONS[h]
        s["compressions_per_s"] = round(N * COMPRESSIONS[h] / (s["median_ms"] * 1e-3))
        res["a_hash_batch_device"][h] = s
        res["b_hash_batch_pinned"][h] = stats(b_sync[h])
        res["b_submit_batch_pinned_rows"][h] = stats(b_ring[h])
        s = stats(c[h])
        s["list_digests_per_s"] = round(n_lists / (s["median_ms"] * 1e-3))
        s["compressions_per_list"] = LIST_COMPRESSIONS[h]
        res["c_digest_lists_device"][h] = s
    print(json.dumps(res))


if __name__ == "__main__":
    main()
