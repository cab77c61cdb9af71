#!/bin/bash
# The measurements of profiles/hasher_plan (run from the repository root on an
# MI355X box after build()):  profiles/hasher_plan/run.sh probe|bench|lanes OUTDIR [LIB]
#   probe: tools/hasher_plan_probe.py -> OUTDIR/hasher_plan_probe.json
#   lanes: tools/hasher_probe.py, LIB against this tree -> OUTDIR/lanes_ab.json
#   bench: the headline, LIB (a libmirsha.so built from the parent commit) and
#          this tree's library alternating, three runs each, the parent first in
#          every round -> OUTDIR/bench_pairs.json (one line per run, "lib" added)
# Every GPU step runs under its own time limit and the script stops at the
# first one that fails.
set -o pipefail
what=$1
out=${2:-.}
mkdir -p "$out"
case "$what" in
probe)
    timeout -k 10 420 python tools/hasher_plan_probe.py > "$out/hasher_plan_probe.json" || exit $?
    ;;
bench)
    parent=$3
    [ -f "$parent" ] || { echo "no parent library at '$parent'" >&2; exit 2; }
    pairs="$out/bench_pairs.json"
    : > "$pairs"
    for round in 1 2 3; do
        for lib in parent this; do
            if [ "$lib" = parent ]; then
                line=$(MIRSHA_AB_LIB="$parent" timeout -k 10 300 python bench.py --gpus 1 --steps 20 --warmup 5 | tail -1) || exit $?
            else
                line=$(timeout -k 10 300 python bench.py --gpus 1 --steps 20 --warmup 5 | tail -1) || exit $?
            fi
            echo "{\"lib\": \"$lib\", \"round\": $round, \"bench\": $line}" >> "$pairs"
        done
    done
    ;;
lanes)
    # tools/hasher_probe.py under LIB and under this tree's library, alternating,
    # two runs each: the two kernels of mirsha_sha512.hip before and after their
    # bodies moved to sha512_lanes.h -> OUTDIR/lanes_ab.json (one line per run)
    parent=$3
    [ -f "$parent" ] || { echo "no parent library at '$parent'" >&2; exit 2; }
    pairs="$out/lanes_ab.json"
    : > "$pairs"
    for round in 1 2; do
        for lib in parent this; do
            if [ "$lib" = parent ]; then
                line=$(MIRSHA_AB_LIB="$parent" timeout -k 10 300 python tools/hasher_probe.py | tail -1) || exit $?
            else
                line=$(timeout -k 10 300 python tools/hasher_probe.py | tail -1) || exit $?
            fi
            echo "{\"lib\": \"$lib\", \"round\": $round, \"probe\": $line}" >> "$pairs"
        done
    done
    ;;
*)
    echo "usage: $0 probe|bench|lanes OUTDIR [LIB]" >&2
    exit 2
    ;;
esac
