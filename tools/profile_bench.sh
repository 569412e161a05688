#!/bin/bash
# GPU box: `rocprofv3 --kernel-trace --stats` over the driver's bench command with every leg on (--full: configs, prg_mode,
# c1_additive and the open step included), the per-kernel summary into <outdir>/<tag>_bench_full_kernel_stats.csv and the line
# into <tag>_bench_profiled.json (bash tools/profile_bench.sh [tag] [outdir], default outdir build/profile).
# The program itself follows `--` (no env/bash hop); no --pmc here (tools/regen_pmc.sh does the counters in passes of their own).
set -o pipefail
R=${GRAFT_REPO_ROOT:-$(cd "$(dirname "$0")/.." && pwd)}
TAG=${1:-r3}
OUT=${2:-build/profile}
export TMPDIR=/tmp
cd "$R" || exit 1
mkdir -p "$OUT" || exit 1
rm -rf "$OUT/prof_stats"
timeout -k 10 600 rocprofv3 --kernel-trace --stats -d "$OUT/prof_stats" --output-format csv -- \
  python3 bench.py --gpus 1 --steps 20 --warmup 5 --full --detail "$OUT/${TAG}_bench_profiled_detail.json" > "$OUT/${TAG}_bench_profiled.json" 2> "$OUT/${TAG}_bench_profiled.err" || exit 2
f=$(find "$OUT/prof_stats" -name "*kernel_stats.csv" | head -1)
[ -n "$f" ] || exit 3
cp "$f" "$OUT/${TAG}_bench_full_kernel_stats.csv"
rm -rf "$OUT/prof_stats"
head -25 "$OUT/${TAG}_bench_full_kernel_stats.csv"
