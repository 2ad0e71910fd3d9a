# usage (on an MI355X node, from anywhere): bash tools/profile_round.sh <tag> [out dir=profile_out]      e.g. r03
# rocprofv3 kernel statistics of the full bench.py run + the bench line itself + PMC traffic of the roofline kernel +
# the other configurations / end-to-end figures of a round; everything lands under <out dir>/<tag>_* (copy what should
# be judged into profiles/).
TAG=$1
OUT=${2:-profile_out}
export TMPDIR=/tmp
cd "$(dirname "$0")/.."
mkdir -p "$OUT"
timeout 900 python bench.py --full > "$OUT/${TAG}_bench.json" 2> "$OUT/${TAG}_bench.err"
# the detail file bench.py names in its line; tools/pmc_traffic.sh writes its files to the same folder
DETAIL=$(tail -1 "$OUT/${TAG}_bench.json" | python -c 'import json, sys; print(json.load(sys.stdin)["detail"])')
RUN_DIR=$(dirname "$DETAIL")
cp "$DETAIL" "$OUT/${TAG}_bench_detail.json"
timeout 900 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/${TAG}_prof" -o p -- python bench.py --full --no-cpu-baseline --no-also > "$OUT/${TAG}_bench_under_rocprof.json" 2> "$OUT/${TAG}_prof.err"
cp "$OUT/${TAG}_prof"/*kernel_stats.csv "$OUT/${TAG}_kernel_stats.csv" 2>/dev/null
TAG=$TAG bash tools/pmc_traffic.sh > "$OUT/${TAG}_pmc_traffic.log" 2>&1
cp "$RUN_DIR/pmc_traffic.json" "$OUT/${TAG}_pmc_traffic_wgrad_ilv.json"
timeout 600 python bench.py --full --config 2 > "$OUT/${TAG}_bench_config2.json" 2>> "$OUT/${TAG}_bench.err"
timeout 600 python bench.py --full --config 5 > "$OUT/${TAG}_bench_config5.json" 2>> "$OUT/${TAG}_bench.err"
( timeout 900 python tools/e2e_train_throughput.py; timeout 900 python tools/e2e_train_throughput.py --from-audio --steps 1000 ) 2>&1 | grep -v amdgpu > "$OUT/${TAG}_e2e.txt"
timeout 600 python tools/step_time_by_dtype.py 2>&1 | grep -v amdgpu > "$OUT/${TAG}_step_time_by_dtype.txt"
timeout 600 python tools/split_by_bucket.py --rule 2>&1 | grep -v amdgpu > "$OUT/${TAG}_split_by_bucket_rule.txt"
timeout 900 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/${TAG}_prof5" -o p -- python bench.py --full --config 5 --no-cpu-baseline > "$OUT/${TAG}_bench_config5_under_rocprof.json" 2>> "$OUT/${TAG}_prof.err"
cp "$OUT/${TAG}_prof5"/*kernel_stats.csv "$OUT/${TAG}_kernel_stats_config5.csv" 2>/dev/null
rm -rf "$OUT/${TAG}_prof" "$OUT/${TAG}_prof5" "$RUN_DIR/pmc_traffic"
tail -1 "$OUT/${TAG}_bench.json" | cut -c1-250
head -12 "$OUT/${TAG}_kernel_stats.csv" | cut -c1-160
