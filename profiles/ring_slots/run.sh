#!/bin/bash
# The measurements of profiles/ring_slots (run from the repository root on an
# MI355X box after build()):  profiles/ring_slots/run.sh WHAT OUTDIR PARENT_LIB [this_first]
#   WHAT = expect_dedup | expect | commit_ring: tools/<WHAT>_probe.py
#          -> OUTDIR/<WHAT>_probe.json, one line per run, "lib" and "round" added
#   WHAT = bench: the headline (bench.py --gpus 1 --steps 20 --warmup 5)
#          -> OUTDIR/bench_pairs.json, likewise
# PARENT_LIB (a libmirsha.so built from the parent commit, loaded through
# MIRSHA_AB_LIB) and this tree's library alternate, three rounds each, the
# parent first in every round; with `this_first` this tree's library first, into
# <name>.this_first.json (the process that runs second in a pair reads a few
# microseconds slower, whichever library it loads: README.txt).  Every GPU step
# runs under its own time limit and the script stops at the first one that fails.
set -o pipefail
what=$1
out=${2:-.}
parent=$3
order="parent this"
suffix=json
[ "${4:-}" = this_first ] && { order="this parent"; suffix=this_first.json; }
[ -f "$parent" ] || { echo "usage: $0 expect_dedup|expect|commit_ring|bench OUTDIR PARENT_LIB [this_first]" >&2; exit 2; }
mkdir -p "$out"
case "$what" in
expect_dedup|expect|commit_ring)
    file="$out/${what}_probe.$suffix"
    run=(python "tools/${what}_probe.py")
    key=probe
    ;;
bench)
    file="$out/bench_pairs.$suffix"
    run=(python bench.py --gpus 1 --steps 20 --warmup 5)
    key=bench
    ;;
*)
    echo "usage: $0 expect_dedup|expect|commit_ring|bench OUTDIR PARENT_LIB [this_first]" >&2
    exit 2
    ;;
esac
: > "$file"
for round in 1 2 3; do
    for lib in $order; do
        if [ "$lib" = parent ]; then
            line=$(MIRSHA_AB_LIB="$parent" timeout -k 10 300 "${run[@]}" | tail -1) || exit $?
        else
            line=$(timeout -k 10 300 "${run[@]}" | tail -1) || exit $?
        fi
        echo "{\"lib\": \"$lib\", \"round\": $round, \"$key\": $line}" >> "$file"
    done
done
