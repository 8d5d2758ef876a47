# Fused vs standalone first_conv A/B on the default bench. Usage: bash tools/ab_fuse_first.sh OUTDIR
set -e
OUT=${1:?OUTDIR}
export PWG_NO_BUILD=1
mkdir -p "$OUT"
for i in 1 2; do
timeout -k 10 300 python bench.py --full --cpu-seconds 0 > "$OUT/fused$i.json" 2> "$OUT/fused$i.err"
timeout -k 10 300 python bench.py --full --cpu-seconds 0 --no-fuse-first > "$OUT/unfused$i.json" 2> "$OUT/unfused$i.err"
done
for f in "$OUT"/*.json; do python -c "import json; d=json.load(open('$f')); print('$f', round(d['value']/1e6,2), d['kernel_ms_per_step'], d['roofline']['avg_launch_ms'])"; done
