#!/bin/bash
# The measurements of profiles/seg_ticket (run from the repository root on an
# MI355X box after build()):  profiles/seg_ticket/run.sh probe|bench OUTDIR PARENT_LIB
# PARENT_LIB: a libmirsha.so built from the parent commit; it and this tree's
# library alternate in one session (MIRSHA_AB_LIB selects the parent's).
#   probe: tools/commit_ring_probe.py and tools/streams_ring_probe.py, each
#          library once per probe (a probe's line carries median, min and max
#          of its 30 timed rounds) -> OUTDIR/probe_pairs.json
#   bench: the headline, three runs each -> OUTDIR/bench_pairs.json
# One line per run, "lib" added.  Every GPU step runs under its own time limit
# and the script stops at the first one that fails.
set -o pipefail
what=$1
out=${2:-.}
parent=$3
mkdir -p "$out"
[ -f "$parent" ] || { echo "no parent library at '$parent'" >&2; exit 2; }

# run LIB SECONDS COMMAND...: the command's last line, under its time limit
run() {
    local lib=$1 limit=$2
    shift 2
    if [ "$lib" = parent ]; then
        MIRSHA_AB_LIB="$parent" timeout -k 10 "$limit" "$@" | tail -1
    else
        timeout -k 10 "$limit" "$@" | tail -1
    fi
}

case "$what" in
probe)
    : > "$out/probe_pairs.json"
    for probe in commit_ring streams_ring; do
        for lib in parent this; do
            line=$(run $lib 400 python tools/${probe}_probe.py) || exit $?
            echo "{\"lib\": \"$lib\", \"result\": $line}" >> "$out/probe_pairs.json"
        done
    done
    ;;
bench)
    : > "$out/bench_pairs.json"
    for round in 1 2 3; do
        for lib in parent this; do
            line=$(run $lib 300 python bench.py --gpus 1 --steps 20 --warmup 5) || exit $?
            echo "{\"lib\": \"$lib\", \"round\": $round, \"bench\": $line}" >> "$out/bench_pairs.json"
        done
    done
    ;;
*)
    echo "usage: $0 probe|bench OUTDIR PARENT_LIB" >&2
    exit 2
    ;;
esac
