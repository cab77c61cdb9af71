#!/bin/bash
# The measurements of profiles/hasher_pair (run from the repository root on an
# MI355X box after build()):  profiles/hasher_pair/run.sh probe|bench OUTDIR LIB
#   LIB: a libmirsha.so built from the parent commit (make -C mirbft_amd/csrc
#        OUT=<dir> in a checkout of it)
#   probe: tools/hasher_pair_probe.py --parent LIB -> OUTDIR/hasher_pair_probe.json
#   bench: the headline, LIB and this tree's library alternating, three runs
#          each, the parent first in every round -> OUTDIR/bench_pairs.json (one
#          line per run, "lib" added)
# Every GPU step runs under its own time limit and the script stops at the
# first one that fails.
set -o pipefail
what=$1
out=${2:-.}
parent=$3
[ -f "$parent" ] || { echo "no parent library at '$parent'" >&2; exit 2; }
mkdir -p "$out"
case "$what" in
probe)
    timeout -k 10 540 python tools/hasher_pair_probe.py --parent "$parent" > "$out/hasher_pair_probe.json" || exit $?
    ;;
bench)
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
*)
    echo "usage: $0 probe|bench OUTDIR LIB" >&2
    exit 2
    ;;
esac
