#!/bin/bash
# The measurements of profiles/list_walker (run from the repository root on an
# MI355X box after build()):  profiles/list_walker/run.sh LEG OUTDIR PARENT_LIB [this_first|trace]
#   LEG = the leg of bench.py that launches one of the kernels whose assembly
#         differs from the parent's (README.txt):
#     headline      sha256_chain_kernel<true>   bench.py --gpus 1 --steps 20 --warmup 5
#     chain_loaded  sha256_chain_kernel<false>  the same with MIRSHA_AB=1 MIRSHA_CHAIN_UNIFORM=0
#     overlap       sha256_msgs_overlap_kernel  ... --pipeline overlap
#     lists         sha256_lists_kernel         ... --pipeline none
#     pair          sha256_chain_pair_kernel    ... --config 3 --pipeline sequential
#   (every leg but the headline adds --timed-kernels all: the batch kernel's own time)
#   -> OUTDIR/bench_<LEG>.json, one line per run, "lib" and "round" added.
# PARENT_LIB (a libmirsha.so built from the parent commit, loaded through
# MIRSHA_AB_LIB) and this tree's library alternate, three rounds each, the
# parent first in every round; with `this_first` this tree's library first, into
# bench_<LEG>.this_first.json.  With `trace`: one rocprofv3 --kernel-trace
# --stats run of the leg per library (the parent first), the sha256 kernels'
# rows of its statistics -> OUTDIR/trace_<LEG>.json.  Every GPU step runs under
# its own time limit and the script stops at the first one that fails.
set -o pipefail
leg=$1
out=${2:-.}
parent=$3
mode=${4:-}
usage() { echo "usage: $0 headline|chain_loaded|overlap|lists|pair OUTDIR PARENT_LIB [this_first|trace]" >&2; exit 2; }
[ -f "$parent" ] || usage
run=(python bench.py --gpus 1 --steps 20 --warmup 5)
knobs=()
case "$leg" in
headline) ;;
chain_loaded) knobs=(MIRSHA_AB=1 MIRSHA_CHAIN_UNIFORM=0); run+=(--timed-kernels all) ;;
overlap) run+=(--pipeline overlap --timed-kernels all) ;;
lists) run+=(--pipeline none --timed-kernels all) ;;
pair) run+=(--config 3 --pipeline sequential --timed-kernels all) ;;
*) usage ;;
esac
mkdir -p "$out"
if [ "$mode" = trace ]; then
    file="$out/trace_$leg.json"
    : > "$file"
    for lib in parent this; do
        dir=$(mktemp -d)
        [ "$lib" = parent ] && ab=(MIRSHA_AB_LIB="$parent") || ab=()
        env "${knobs[@]}" "${ab[@]}" timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv \
            -d "$dir" -o run -- "${run[@]}" > /dev/null || exit $?
        stats=$(find "$dir" -name '*kernel_stats.csv' | head -1)
        python - "$stats" "$lib" "$leg" >> "$file" <<'EOF' || exit $?
import csv, json, sys
rows = {r["Name"].split("(")[0].replace("void ", ""): {"calls": int(r["Calls"]), "avg_us": float(r["AverageNs"]) / 1e3,
                                                        "min_us": float(r["MinNs"]) / 1e3, "max_us": float(r["MaxNs"]) / 1e3}
        for r in csv.DictReader(open(sys.argv[1])) if "sha256" in r["Name"]}
print(json.dumps({"lib": sys.argv[2], "leg": sys.argv[3], "kernels": rows}))
EOF
        rm -r "$dir"
    done
    exit 0
fi
order="parent this"
suffix=json
[ "$mode" = this_first ] && { order="this parent"; suffix=this_first.json; }
file="$out/bench_$leg.$suffix"
: > "$file"
for round in 1 2 3; do
    for lib in $order; do
        [ "$lib" = parent ] && ab=(MIRSHA_AB_LIB="$parent") || ab=()
        line=$(env "${knobs[@]}" "${ab[@]}" timeout -k 10 300 "${run[@]}" | tail -1) || exit $?
        echo "{\"lib\": \"$lib\", \"round\": $round, \"bench\": $line}" >> "$file"
    done
done
