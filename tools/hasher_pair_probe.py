#!/usr/bin/env python3
"""The SHA-512/256 producer/consumer pair route against the one-lane kernels:
one JSON line.

One process on one MI355X, the legs interleaved round by round, 5 warm-up and
30 timed rounds, medians with min-max; every round's digests are compared with
hashlib in full.  Timed by the context's kernel timers (ids 0 and 1).  Measured,
not gated.

Legs of every shape:
    parent    the library given with --parent (a libmirsha.so built from the
              parent commit: the one-lane kernels as they were), loaded beside
              this tree's in the same process.  THE reference.
    pair      this tree, the automatic route (variant 6 where the shape lies
              above the threshold, said in "forced")
    one_lane  this tree with set_variant(5): message shapes only (the list
              launches have no variant; their in-process A/B is the knob
              MIRSHA_AB=1 MIRSHA_SHA512_PAIR=0, read once per process)

Shapes: 64 messages of 61,600 B (482 dependent blocks a lane); 9 lists of up to
500 through mirsha_digest_lists_device and through a sequential plan; the
config-1 cycle (16 x 33 B, then one list of 16); 1,000 x 272 B; then 33 B and
4 KiB messages at 1, 64, 256, 384 and 512 groups of 64 (above the threshold the
pair leg is variant 6).

Usage (GPU box):  python tools/hasher_pair_probe.py --parent PATH/libmirsha.so
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

WARM, TIMED = 5, 30
HASHER = "sha512_256"


def H(b) -> bytes:
    return hashlib.new(HASHER, bytes(b)).digest()


def stats(v):
    return {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(np.min(v)), 4),
            "max_ms": round(float(np.max(v)), 4)}


def rounds(legs):
    """legs: name -> callable() -> {figure: ms}; interleaved, warm-up dropped."""
    got = {k: {} for k in legs}
    for r in range(WARM + TIMED):
        for k, leg in legs.items():
            figures = leg()
            if r >= WARM:
                for f, ms in figures.items():
                    got[k].setdefault(f, []).append(ms)
    return {k: {f: stats(v) for f, v in fs.items()} for k, fs in got.items()}


def blocks(length: int) -> int:
    return (length + 16) // 128 + 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="libmirsha.so built from the parent commit")
    args = ap.parse_args()
    import torch

    assert torch.cuda.is_available()
    from mirbft_amd import Engine, _lib, sha512_pair_max_groups
    from mirbft_amd.engine import KERNEL_LISTS, KERNEL_MSGS

    this = Engine(0)
    # the parent's library beside this tree's: a second copy under another path,
    # its engine keeps it (Engine._lib); the module's own handle is put back
    mine = _lib._lib
    _lib._lib, os.environ["MIRSHA_AB_LIB"] = None, args.parent
    try:
        parent = Engine(0)
    finally:
        _lib._lib = mine
        del os.environ["MIRSHA_AB_LIB"]
    assert parent._lib is not this._lib and not hasattr(parent._lib, "mirsha_ctx_sha512_pair_launches")
    for e in (this, parent):
        e.set_hasher(HASHER)
        e.set_timing(True)
    threshold = sha512_pair_max_groups()

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def timed(eng, call, ids):
        eng.reset_timing()
        call()
        eng.sync()
        t = {k: eng.kernel_time(k) for k in ids}
        assert all(n == 1 for n, _ in t.values()), t
        return {k: ms for k, (n, ms) in t.items()}

    def message_legs(n, size, seed):
        rng = np.random.default_rng(seed)
        arena = rng.integers(0, 256, size=n * size, dtype=np.uint8)
        want = np.frombuffer(b"".join(H(arena[i * size:(i + 1) * size]) for i in range(n)), dtype=np.uint8)
        d_arena = dev(arena)
        d_off = dev((np.arange(n, dtype=np.uint64) * size).view(np.int64))
        d_len = dev(np.full(n, size, dtype=np.uint32).view(np.int32))
        d_out = torch.zeros((n, 32), dtype=torch.uint8, device="cuda")
        forced = (n + 63) // 64 > threshold

        def leg(eng, variant, pair_launches):
            def run():
                d_out.zero_()
                torch.cuda.synchronize()
                eng.set_variant(variant)
                before = eng.sha512_pair_launches if eng is this else 0
                t = timed(eng, lambda: eng.hash_batch_device(d_arena.data_ptr(), n * size, d_off.data_ptr(),
                                                             d_len.data_ptr(), None, n, d_out.data_ptr()),
                          (KERNEL_MSGS,))
                eng.set_variant(0)
                if eng is this:
                    assert eng.sha512_pair_launches - before == pair_launches
                if d_out.cpu().numpy().tobytes() != want.tobytes():
                    raise SystemExit(f"{n} x {size} B: digests differ from hashlib")
                return {"request_kernel": t[KERNEL_MSGS]}
            return run
        legs = {"parent": leg(parent, 0, 0), "pair": leg(this, 6 if forced else 0, 1), "one_lane": leg(this, 5, 0)}
        return legs, {"n": n, "bytes": size, "groups": (n + 63) // 64, "dependent_blocks": blocks(size),
                      "forced": forced}

    def finish(meta, got):
        dep = meta["dependent_blocks"]
        for k, figures in got.items():
            for f, s in figures.items():
                if f in ("request_kernel", "list_kernel"):
                    s["us_per_dependent_block"] = round(1e3 * s["median_ms"] / dep[f] if isinstance(dep, dict)
                                                        else 1e3 * s["median_ms"] / dep, 3)
        p, q = got["parent"], got["pair"]
        f = "list_kernel" if "list_kernel" in q and "request_kernel" not in q else "request_kernel"
        meta["pair_median_below_parent_min"] = {k: q[k]["median_ms"] < p[k]["min_ms"] for k in q if k != "wall"}
        meta["pair_over_parent"] = round(q[f]["median_ms"] / p[f]["median_ms"], 4)
        return {**meta, **got}

    res = {"device": torch.cuda.get_device_name(0), "warmup_rounds": WARM, "timed_rounds": TIMED,
           "threshold_groups": threshold}

    # 64 x 61,600 B and 1,000 x 272 B
    for name, n, size, seed in (("msgs_64x61600", 64, 61_600, 1), ("msgs_1000x272", 1000, 272, 2)):
        legs, meta = message_legs(n, size, seed)
        res[name] = finish(meta, rounds(legs))
        torch.cuda.empty_cache()

    # 9 lists of up to 500: the call, and a sequential plan over the same lists
    rng = np.random.default_rng(3)
    n_req, size = 4096, 64
    counts = [500] * 8 + [96]
    idx = np.arange(n_req, dtype=np.uint32)
    first = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
    arena = rng.integers(0, 256, size=n_req * size, dtype=np.uint8)
    req = [H(arena[i * size:(i + 1) * size]) for i in range(n_req)]
    want_req = np.frombuffer(b"".join(req), dtype=np.uint8)
    want_bat = np.frombuffer(b"".join(H(b"".join(req[first[b]:first[b + 1]])) for b in range(9)), dtype=np.uint8)
    d_arena, d_off = dev(arena), dev((np.arange(n_req, dtype=np.uint64) * size).view(np.int64))
    d_len = dev(np.full(n_req, size, dtype=np.uint32).view(np.int32))
    d_idx, d_first, d_table = dev(idx.view(np.int32)), dev(first.view(np.int32)), dev(want_req.reshape(-1, 32))
    d_req = torch.zeros((n_req, 32), dtype=torch.uint8, device="cuda")
    d_bat = torch.zeros((9, 32), dtype=torch.uint8, device="cuda")

    def lists_leg(eng):
        def run():
            d_bat.zero_()
            torch.cuda.synchronize()
            t = timed(eng, lambda: eng.digest_lists_device(d_table.data_ptr(), n_req, d_idx.data_ptr(),
                                                           d_first.data_ptr(), 9, n_req, d_bat.data_ptr()),
                      (KERNEL_LISTS,))
            if d_bat.cpu().numpy().tobytes() != want_bat.tobytes():
                raise SystemExit("9 lists: digests differ from hashlib")
            return {"list_kernel": t[KERNEL_LISTS]}
        return run
    got = rounds({"parent": lists_leg(parent), "pair": lists_leg(this)})
    res["lists_9_of_500_call"] = finish({"n_lists": 9, "entries": counts, "dependent_blocks": 500 // 4 + 1}, got)

    plans = {"parent": parent.pipeline(n_req, idx, first, np.full(n_req, size, dtype=np.uint32), mode="sequential",
                                       hasher=HASHER),
             "pair": this.pipeline(n_req, idx, first, np.full(n_req, size, dtype=np.uint32), mode="sequential",
                                   hasher=HASHER)}

    def plan_leg(eng, plan):
        def run():
            d_req.zero_()
            d_bat.zero_()
            torch.cuda.synchronize()
            t = timed(eng, lambda: eng.hash_requests_then_batches_device(plan, d_arena.data_ptr(), n_req * size,
                                                                         d_off.data_ptr(), d_len.data_ptr(),
                                                                         d_req.data_ptr(), d_bat.data_ptr()),
                      (KERNEL_MSGS, KERNEL_LISTS))
            if d_req.cpu().numpy().tobytes() != want_req.tobytes() or d_bat.cpu().numpy().tobytes() != want_bat.tobytes():
                raise SystemExit("plan over 9 lists: digests differ from hashlib")
            return {"request_kernel": t[KERNEL_MSGS], "list_kernel": t[KERNEL_LISTS]}
        return run
    got = rounds({"parent": plan_leg(parent, plans["parent"]), "pair": plan_leg(this, plans["pair"])})
    res["lists_9_of_500_plan"] = finish({"n_req": n_req, "request_bytes": size, "n_lists": 9, "entries": counts,
                                         "dependent_blocks": {"request_kernel": blocks(size),
                                                              "list_kernel": 500 // 4 + 1}}, got)
    for p in plans.values():
        p.close()

    # the config-1 cycle: 16 x 33 B, then one list of the 16 digests
    rng = np.random.default_rng(4)
    a1 = rng.integers(0, 256, size=16 * 33, dtype=np.uint8)
    r1 = [H(a1[i * 33:(i + 1) * 33]) for i in range(16)]
    w1r, w1b = b"".join(r1), H(b"".join(r1))
    d_a1, d_o1 = dev(a1), dev((np.arange(16, dtype=np.uint64) * 33).view(np.int64))
    d_l1 = dev(np.full(16, 33, dtype=np.uint32).view(np.int32))
    d_i1, d_f1 = dev(np.arange(16, dtype=np.int32)), dev(np.array([0, 16], dtype=np.int32))
    d_r1 = torch.zeros((16, 32), dtype=torch.uint8, device="cuda")
    d_b1 = torch.zeros((1, 32), dtype=torch.uint8, device="cuda")

    def cycle_leg(eng):
        def call():
            eng.hash_batch_device(d_a1.data_ptr(), 16 * 33, d_o1.data_ptr(), d_l1.data_ptr(), None, 16, d_r1.data_ptr())
            eng.digest_lists_device(d_r1.data_ptr(), 16, d_i1.data_ptr(), d_f1.data_ptr(), 1, 16, d_b1.data_ptr())

        def run():
            d_r1.zero_()
            d_b1.zero_()
            torch.cuda.synchronize()
            t = timed(eng, call, (KERNEL_MSGS, KERNEL_LISTS))
            if d_r1.cpu().numpy().tobytes() != w1r or d_b1.cpu().numpy().tobytes() != w1b:
                raise SystemExit("config-1 cycle: digests differ from hashlib")
            return {"request_kernel": t[KERNEL_MSGS], "list_kernel": t[KERNEL_LISTS],
                    "kernels": t[KERNEL_MSGS] + t[KERNEL_LISTS]}
        return run
    got = rounds({"parent": cycle_leg(parent), "pair": cycle_leg(this)})
    res["config1_cycle"] = finish({"requests": 16, "request_bytes": 33, "list_entries": 16,
                                   "dependent_blocks": {"request_kernel": 1, "list_kernel": 5}}, got)

    # the group-count sweep
    sweep = {}
    for size in (33, 4096):
        for g in (1, 64, 256, 384, 512):
            legs, meta = message_legs(64 * g, size, 100 * g + size)
            sweep[f"{size}B_x_{g}_groups"] = finish(meta, rounds(legs))
            torch.cuda.empty_cache()
    res["sweep"] = sweep

    for e in (this, parent):
        e.set_timing(False)
        e.set_hasher("sha256")
        e.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
