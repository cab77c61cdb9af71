#!/bin/bash
# The measurements of profiles/streams_ring (run from the repository root on an
# MI355X box after build()):  profiles/streams_ring/run.sh probe|bench OUTDIR [PARENT_LIB]
#   probe: tools/streams_ring_probe.py -> OUTDIR/streams_ring_probe.json
#   bench: the headline, PARENT_LIB (a libmirsha.so built from the parent
#          commit) and this tree's library alternating, three runs each
#          -> OUTDIR/bench_pairs.json (one line per run, "lib" added)
# Every GPU step runs under its own time limit and the script stops at the
# first one that fails.
set -o pipefail
what=$1
out=${2:-.}
mkdir -p "$out"
case "$what" in
probe)
    timeout -k 10 400 python tools/streams_ring_probe.py > "$out/streams_ring_probe.json" || exit $?
    ;;
bench)
    parent=$3
    [ -f "$parent" ] || { echo "no parent library at '$parent'" >&2; exit 2; }
    : > "$out/bench_pairs.json"
    for round in 1 2 3; do
        for lib in parent this; do
            if [ "$lib" = parent ]; then
                line=$(MIRSHA_AB_LIB="$parent" timeout -k 10 300 python bench.py --gpus 1 --steps 20 --warmup 5 | tail -1) || exit $?
            else
                line=$(timeout -k 10 300 python bench.py --gpus 1 --steps 20 --warmup 5 | tail -1) || exit $?
            fi
            echo "{\"lib\": \"$lib\", \"round\": $round, \"bench\": $line}" >> "$out/bench_pairs.json"
        done
    done
    ;;
*)
    echo "usage: $0 probe|bench OUTDIR [PARENT_LIB]" >&2
    exit 2
    ;;
esac
