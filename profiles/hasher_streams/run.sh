#!/bin/bash
# The measurements of profiles/hasher_streams (run from the repository root on an
# MI355X box after build()):  profiles/hasher_streams/run.sh probe|bench OUTDIR [LIB [FIRST]]
#   probe: tools/hasher_streams_probe.py -> OUTDIR/hasher_streams_probe.json
#   bench: the headline, LIB (a libmirsha.so built from the parent commit) and
#          this tree's library alternating, three runs each, FIRST (parent, the
#          default, or this) going first in every round
#          -> OUTDIR/bench_pairs.json, or bench_pairs_this_first.json
#          (one line per run, "lib" added)
# Every GPU step runs under its own time limit and the script stops at the
# first one that fails.
set -o pipefail
what=$1
out=${2:-.}
mkdir -p "$out"
case "$what" in
probe)
    timeout -k 10 420 python tools/hasher_streams_probe.py > "$out/hasher_streams_probe.json" || exit $?
    ;;
bench)
    parent=$3
    [ -f "$parent" ] || { echo "no parent library at '$parent'" >&2; exit 2; }
    order="parent this"
    pairs="$out/bench_pairs.json"
    if [ "${4:-parent}" = this ]; then
        order="this parent"
        pairs="$out/bench_pairs_this_first.json"
    fi
    : > "$pairs"
    for round in 1 2 3; do
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
    echo "usage: $0 probe|bench OUTDIR [LIB [FIRST]]" >&2
    exit 2
    ;;
esac
