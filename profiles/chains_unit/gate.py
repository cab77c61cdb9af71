#!/usr/bin/env python3
"""The speed gate of profiles/chains_unit over run.sh's two files:

    python profiles/chains_unit/gate.py [DIR]

For each figure the six lines (parent and this tree, three rounds each), and
the gate: this tree's median no higher than the parent's maximum."""
import json
import os
import statistics
import sys

HERE = sys.argv[1] if len(sys.argv) > 1 else os.path.dirname(os.path.abspath(__file__))
FIGURES = [  # (file, label, path into the probe's JSON line)
    ("commit_probe.json", "chains_commit_kernel, checkpoints_1: kernels.one_call.device_ms",
     ("checkpoints_1", "kernels", "one_call", "device_ms")),
    ("commit_probe.json", "chains_commit_kernel, checkpoints_4: kernels.one_call.device_ms",
     ("checkpoints_4", "kernels", "one_call", "device_ms")),
    ("commit_ring_probe.json", "chains_commit_seg_kernel, checkpoints_1: kernel.device_ms median",
     ("kernel", "checkpoints_1", "device_ms", "chains_commit_seg_kernel", "median")),
    ("commit_ring_probe.json", "chains_commit_seg_kernel, checkpoints_4: kernel.device_ms median",
     ("kernel", "checkpoints_4", "device_ms", "chains_commit_seg_kernel", "median")),
]


def main():
    status = 0
    print("| figure (ms) | parent, rounds 1-3 | parent max | this tree, rounds 1-3 | this tree, median | gate |")
    print("|---|---|---|---|---|---|")
    for name, label, path in FIGURES:
        vals = {"parent": [], "this": []}
        for line in open(os.path.join(HERE, name)):
            rec = json.loads(line)
            v = rec["probe"]
            for k in path:
                v = v[k]
            vals[rec["lib"]].append(float(v))
        pmax, med = max(vals["parent"]), statistics.median(vals["this"])
        ok = med <= pmax
        status |= not ok
        fmt = lambda xs: ", ".join(f"{x:.4f}" for x in xs)
        print(f"| {label} | {fmt(vals['parent'])} | {pmax:.4f} | {fmt(vals['this'])} | {med:.4f} | "
              f"{'met' if ok else f'MISSED by {med - pmax:.4f}'} |")
    return status


if __name__ == "__main__":
    sys.exit(main())
