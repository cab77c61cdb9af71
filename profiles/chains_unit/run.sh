#!/bin/bash
# The measurements of profiles/chains_unit (run from the repository root on an
# MI355X box after build()):  profiles/chains_unit/run.sh ab|bench|bench_ab OUTDIR [LIB]
#   ab:    the two commit probes, LIB (a libmirsha.so built from the parent
#          commit, loaded with MIRSHA_AB_LIB) and this tree's library
#          alternating, three rounds, the parent first in every round, one
#          probe a process -> OUTDIR/commit_probe.json, OUTDIR/commit_ring_probe.json
#          (one line per run, "lib" and "round" added).  commit_ring_probe runs
#          with --small: its "kernel" leg, the one read here, is the same in
#          both forms; the option only shrinks the hashing cycles of its other legs.
#   bench: the headline once -> OUTDIR/bench_headline.json
#   bench_ab: the headline, LIB and this tree's library alternating, three
#          rounds, the parent first -> OUTDIR/bench_pairs.json
# Every GPU step runs under its own time limit and the script stops at the
# first one that fails.
set -o pipefail
what=$1
out=${2:-.}
mkdir -p "$out"
case "$what" in
ab)
    parent=$3
    [ -f "$parent" ] || { echo "no parent library at '$parent'" >&2; exit 2; }
    : > "$out/commit_probe.json"
    : > "$out/commit_ring_probe.json"
    for round in 1 2 3; do
        for lib in parent this; do
            for probe in commit_probe commit_ring_probe; do
                args=
                [ "$probe" = commit_ring_probe ] && args=--small
                if [ "$lib" = parent ]; then
                    line=$(MIRSHA_AB_LIB="$parent" timeout -k 10 300 python tools/$probe.py $args | tail -1) || exit $?
                else
                    line=$(timeout -k 10 300 python tools/$probe.py $args | tail -1) || exit $?
                fi
                echo "{\"lib\": \"$lib\", \"round\": $round, \"probe\": $line}" >> "$out/$probe.json"
                echo "$probe $lib $round done"
            done
        done
    done
    ;;
bench)
    timeout -k 10 300 python bench.py --gpus 1 --steps 20 --warmup 5 | tail -1 > "$out/bench_headline.json" || exit $?
    cat "$out/bench_headline.json"
    ;;
bench_ab)
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
    echo "usage: $0 ab|bench|bench_ab OUTDIR [LIB]" >&2
    exit 2
    ;;
esac
