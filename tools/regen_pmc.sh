#!/bin/bash
# GPU box: the two PMC passes behind profiles/pmc_traffic.json, then the file itself (into the output directory, the first
# argument, default build/pmc; copy it to profiles/).  bench.py --full: the side configurations and the k_copy16 probe the
# passes read run only there.
# rocprofv3 gets the program itself after `--` (no env/bash hop), and --pmc is never combined with a trace domain.
set -o pipefail
R=${GRAFT_REPO_ROOT:-$(cd "$(dirname "$0")/.." && pwd)}
export TMPDIR=/tmp
cd "$R" || exit 1
OUT=${1:-build/pmc}
mkdir -p "$OUT" || exit 1
rm -rf "$OUT/pmc_fetch" "$OUT/pmc_write"
timeout -k 10 500 rocprofv3 --pmc FETCH_SIZE -d "$OUT/pmc_fetch" --output-format csv -- \
  python3 bench.py --full --open 0 --cpu-sample 0 --ew 0 --steps 5 --pmc-live 0 --detail "$OUT/pmc_fetch_detail.json" > "$OUT/pmc_fetch.json" 2> "$OUT/pmc_fetch.err" || exit 2
timeout -k 10 500 rocprofv3 --pmc WRITE_SIZE -d "$OUT/pmc_write" --output-format csv -- \
  python3 bench.py --full --open 0 --cpu-sample 0 --ew 0 --steps 5 --pmc-live 0 --detail "$OUT/pmc_write_detail.json" > "$OUT/pmc_write.json" 2> "$OUT/pmc_write.err" || exit 3
python3 tools/make_pmc_traffic.py "$OUT/pmc_fetch" "$OUT/pmc_write" 4000000000 > "$OUT/pmc_traffic.json" || exit 4
# the raw counter CSVs are large; keep only the summary
rm -rf "$OUT/pmc_fetch" "$OUT/pmc_write"
cat "$OUT/pmc_traffic.json"
