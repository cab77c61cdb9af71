#!/usr/bin/env python3
"""The device plans under the two hashers side by side: one JSON line.

One process on one MI355X, the legs interleaved round by round, 5 warm-up and
30 timed rounds, medians with min-max; every round's request and batch digests
are spot-checked against hashlib.  Measured, not gated.

Leg (a): the config-2 shape, 2^20 requests of 272 B on the device, 52,429
  identity batches of 20, under each hasher:
    plan      the sequential plan (mirsha_pipeline_create_hasher,
              mirsha_hash_requests_then_batches_device): the request kernel
              (timing id 0), the list kernel (id 1), their sum, the call's wall
              time to the synchronised end
    overlap   the overlapped stream (mirsha_pipeline_overlap_device), one
              steady-state cycle per round: its one launch (id 5) and wall time
    calls     mirsha_hash_batch_device + mirsha_digest_lists_device, the only
              way before the plans followed the hasher (ids 0 and 1)
Leg (b): the list kernels of SHA-512/256 on that list shape, each behind the
  same request launch: sha512_plan_lists_kernel<true> (the uniform plan),
  <false> (the same plan created with MIRSHA_AB=1 MIRSHA_CHAIN_UNIFORM=0) and
  sha512_lists_kernel (mirsha_digest_lists_device).
Leg (c): one config-3-like shape, 2^12 requests of 4 KiB, 9 lists of up to 500:
  the SHA-512/256 sequential plan and overlapped cycle, and the SHA-256 plan
  AUTO picks, per step.

Usage (GPU box):  python tools/hasher_plan_probe.py
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


def stats(v):
    return {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(np.min(v)), 4),
            "max_ms": round(float(np.max(v)), 4)}


def oracle(name, b):
    return hashlib.new(name, bytes(b)).digest()


def rounds(legs):
    """legs: name -> callable(round) -> {figure: ms}; interleaved, warm-up dropped."""
    got = {k: {} for k in legs}
    for r in range(WARM + TIMED):
        for k, leg in legs.items():
            figures = leg(r)
            if r >= WARM:
                for f, ms in figures.items():
                    got[k].setdefault(f, []).append(ms)
    return {k: {f: stats(v) for f, v in fs.items()} for k, fs in got.items()}


class Shape:
    """n requests of `size` bytes on the device and identity lists of `batch`."""

    def __init__(self, torch, sharding, n, size, batch, seed):
        rng = np.random.default_rng(seed)
        self.n, self.size, self.batch = n, size, batch
        self.arena = rng.integers(0, 256, size=n * size, dtype=np.uint8)
        self.off = np.arange(n, dtype=np.uint64) * size
        self.ln = np.full(n, size, dtype=np.uint32)
        self.idx, self.first = sharding.batch_lists(n, batch)
        self.n_lists = int(self.first.size) - 1
        self.d_arena = torch.from_numpy(self.arena).cuda()
        self.d_off = torch.from_numpy(self.off.view(np.int64)).cuda()
        self.d_len = torch.from_numpy(self.ln.view(np.int32)).cuda()
        self.d_idx = torch.from_numpy(self.idx.view(np.int32)).cuda()
        self.d_first = torch.from_numpy(self.first.view(np.int32)).cuda()
        self.d_req = [torch.zeros((n, 32), dtype=torch.uint8, device="cuda") for _ in range(2)]
        self.d_bat = torch.zeros((self.n_lists, 32), dtype=torch.uint8, device="cuda")
        self.spots = rng.integers(0, n, size=(WARM + TIMED, 4))
        self.want = {}
        self.torch = torch

    @property
    def args(self):
        return self.d_arena.data_ptr(), self.n * self.size, self.d_off.data_ptr(), self.d_len.data_ptr()

    def clear(self, *tensors):
        for t in tensors:
            t.zero_()
        self.torch.cuda.synchronize()  # torch's stream vs the engine's own

    def request_digest(self, h, i):
        if (h, "r", i) not in self.want:
            self.want[(h, "r", i)] = oracle(h, self.arena[i * self.size:(i + 1) * self.size])
        return self.want[(h, "r", i)]

    def batch_digest(self, h, b):
        if (h, "b", b) not in self.want:
            lo, hi = b * self.batch, min((b + 1) * self.batch, self.n)
            self.want[(h, "b", b)] = oracle(h, b"".join(self.request_digest(h, i) for i in range(lo, hi)))
        return self.want[(h, "b", b)]

    def check(self, h, r, d_req, d_bat, what):
        """Four request digests and the batch digest of the first one's batch
        (plus the last, partial or not) against hashlib."""
        if d_req is not None:
            got = d_req[self.torch.from_numpy(self.spots[r])].cpu().numpy()
            for k, i in enumerate(self.spots[r]):
                if got[k].tobytes() != self.request_digest(h, int(i)):
                    raise SystemExit(f"{what} {h}: request digest {int(i)} differs from hashlib in round {r}")
        if d_bat is not None:
            for b in (int(self.spots[r][0]) // self.batch, self.n_lists - 1):
                if d_bat[b].cpu().numpy().tobytes() != self.batch_digest(h, b):
                    raise SystemExit(f"{what} {h}: batch digest {b} differs from hashlib in round {r}")


def main():
    import torch

    assert torch.cuda.is_available()
    from mirbft_amd import Engine, sharding
    from mirbft_amd.engine import KERNEL_FUSED, KERNEL_LISTS, KERNEL_MSGS, KERNEL_OVERLAP

    eng = Engine(0)
    eng.set_timing(True)

    def timed(h, call):
        """(launches and ms per timing id, wall ms) of one call to its synchronised end."""
        eng.set_hasher(h)
        eng.reset_timing()
        t0 = time.perf_counter()
        call()
        eng.sync()
        wall = (time.perf_counter() - t0) * 1e3
        return {k: eng.kernel_time(k) for k in (KERNEL_MSGS, KERNEL_LISTS, KERNEL_FUSED, KERNEL_OVERLAP)}, wall

    def plan_leg(s, h, plan):
        def leg(r):
            s.clear(s.d_req[0], s.d_bat)
            t, wall = timed(h, lambda: eng.hash_requests_then_batches_device(plan, *s.args, s.d_req[0].data_ptr(),
                                                                            s.d_bat.data_ptr()))
            s.check(h, r, s.d_req[0], s.d_bat, "plan")
            if plan.mode_name == "fused":
                assert (t[KERNEL_MSGS][0], t[KERNEL_LISTS][0], t[KERNEL_FUSED][0]) == (0, 0, 1), t
                return {"fused_kernel": t[KERNEL_FUSED][1], "wall": wall}
            assert (t[KERNEL_MSGS][0], t[KERNEL_LISTS][0], t[KERNEL_FUSED][0]) == (1, 1, 0), t
            return {"request_kernel": t[KERNEL_MSGS][1], "list_kernel": t[KERNEL_LISTS][1],
                    "kernels": t[KERNEL_MSGS][1] + t[KERNEL_LISTS][1], "wall": wall}
        return leg

    def overlap_leg(s, h, plan):
        # the stream's own two request-digest buffers: a cycle's lists read what
        # the cycle before wrote, whatever the other legs ran in between
        state = {"i": 0, "req": [torch.zeros_like(s.d_req[0]) for _ in range(2)]}

        def leg(r):
            i = state["i"]
            cur, prev = state["req"][i % 2], state["req"][(i - 1) % 2]
            if i == 0:  # the stream's first cycle, tiles only, outside the figures
                timed(h, lambda: eng.pipeline_overlap_device(plan, *s.args, prev.data_ptr(), 0, 0))
            s.clear(cur, s.d_bat)
            t, wall = timed(h, lambda: eng.pipeline_overlap_device(plan, *s.args, cur.data_ptr(), prev.data_ptr(),
                                                                   s.d_bat.data_ptr()))
            state["i"] = i + 1
            s.check(h, r, cur, s.d_bat, "overlap")
            which = KERNEL_FUSED if plan.mode_name == "fused" else KERNEL_OVERLAP
            assert t[which][0] == 1 and t[KERNEL_MSGS][0] == 0 and t[KERNEL_LISTS][0] == 0, t
            return {"kernel": t[which][1], "wall": wall}
        return leg

    def calls_leg(s, h):
        def leg(r):
            s.clear(s.d_req[0], s.d_bat)

            def call():
                eng.hash_batch_device(*s.args, None, s.n, s.d_req[0].data_ptr())
                eng.digest_lists_device(s.d_req[0].data_ptr(), s.n, s.d_idx.data_ptr(), s.d_first.data_ptr(),
                                        s.n_lists, int(s.idx.size), s.d_bat.data_ptr())
            t, wall = timed(h, call)
            s.check(h, r, s.d_req[0], s.d_bat, "calls")
            assert (t[KERNEL_MSGS][0], t[KERNEL_LISTS][0]) == (1, 1), t
            return {"request_kernel": t[KERNEL_MSGS][1], "list_kernel": t[KERNEL_LISTS][1],
                    "kernels": t[KERNEL_MSGS][1] + t[KERNEL_LISTS][1], "wall": wall}
        return leg

    def make_plan(s, h, loaded_indices=False):
        if loaded_indices:  # the A/B knob of uniform_lists(): the same lists, indices loaded
            os.environ["MIRSHA_AB"], os.environ["MIRSHA_CHAIN_UNIFORM"] = "1", "0"
        try:
            return eng.pipeline(s.n, s.idx, s.first, s.ln, hasher=h)
        finally:
            if loaded_indices:
                del os.environ["MIRSHA_AB"], os.environ["MIRSHA_CHAIN_UNIFORM"]

    res = {"device": torch.cuda.get_device_name(0), "warmup_rounds": WARM, "timed_rounds": TIMED}

    # (a) and (b): config 2's shape
    s = Shape(torch, sharding, 1 << 20, 272, 20, 41)
    plans = {h: make_plan(s, h) for h in HASHERS}
    loaded = make_plan(s, "sha512_256", loaded_indices=True)
    legs = {}
    for h in HASHERS:
        legs[f"plan/{h}"] = plan_leg(s, h, plans[h])
        legs[f"overlap/{h}"] = overlap_leg(s, h, plans[h])
        legs[f"calls/{h}"] = calls_leg(s, h)
    legs["plan_loaded_indices/sha512_256"] = plan_leg(s, "sha512_256", loaded)
    got = rounds(legs)
    res["a_config2"] = {"n": s.n, "request_bytes": s.size, "batch": s.batch, "n_lists": s.n_lists,
                        "plan_modes": {h: plans[h].mode_name for h in HASHERS},
                        **{k: v for k, v in got.items() if not k.startswith("plan_loaded")}}
    res["b_list_kernels_sha512_256"] = {
        "sha512_plan_lists_kernel<true>": got["plan/sha512_256"]["list_kernel"],
        "sha512_plan_lists_kernel<false>": got["plan_loaded_indices/sha512_256"]["list_kernel"],
        "sha512_lists_kernel": got["calls/sha512_256"]["list_kernel"]}
    for p in list(plans.values()) + [loaded]:
        p.close()
    del s
    torch.cuda.empty_cache()

    # (c): a config-3-like shape
    s = Shape(torch, sharding, 1 << 12, 4096, 500, 43)
    plans = {h: make_plan(s, h) for h in HASHERS}
    legs = {}
    for h in HASHERS:
        legs[f"plan/{h}"] = plan_leg(s, h, plans[h])
        legs[f"overlap/{h}"] = overlap_leg(s, h, plans[h])
    res["c_config3_like"] = {"n": s.n, "request_bytes": s.size, "batch": s.batch, "n_lists": s.n_lists,
                             "plan_modes": {h: plans[h].mode_name for h in HASHERS}, **rounds(legs)}
    for p in plans.values():
        p.close()
    eng.set_timing(False)
    eng.set_hasher("sha256")
    eng.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
