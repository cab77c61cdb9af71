#!/bin/bash
# The measurements of profiles/hasher_chains_pair (run from the repository root
# on an MI355X box after build()):  profiles/hasher_chains_pair/run.sh probe|bench OUTDIR [LIB]
#   probe: tools/hasher_chains_pair_probe.py -> OUTDIR/hasher_chains_pair_probe.json
#          (both legs are this tree's library: set_variant(5) and set_variant(6))
#   bench: the headline, LIB (a libmirsha.so built from the parent commit: make
#          -C mirbft_amd/csrc OUT=<dir> in a checkout of it) and this tree's
#          library alternating, three runs each, the order alternating from round
#          to round -> OUTDIR/bench_pairs.json (one line per run, "lib" added)
# Every GPU step runs under its own time limit and the script stops at the
# first one that fails.
set -o pipefail
what=$1
out=${2:-.}
parent=$3
mkdir -p "$out"
case "$what" in
probe)
    timeout -k 10 540 python tools/hasher_chains_pair_probe.py > "$out/hasher_chains_pair_probe.json" || exit $?
    ;;
bench)
    [ -f "$parent" ] || { echo "no parent library at '$parent'" >&2; exit 2; }
    pairs="$out/bench_pairs.json"
    : > "$pairs"
    for round in 1 2 3; do
        if [ $((round % 2)) = 1 ]; then order="parent this"; else order="this parent"; fi
        for lib in $order; do
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
    echo "usage: $0 probe|bench OUTDIR [LIB]" >&2
    exit 2
    ;;
esac
