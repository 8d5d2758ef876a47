# The bench batch as k sequential sub-batches. Usage: bash tools/diag/subplans.sh OUTDIR
set -e
OUT=${1:?OUTDIR}
export PWG_NO_BUILD=1
mkdir -p "$OUT"
for k in 1 32 16 8 4 2 1 32; do
  timeout -k 10 200 python bench.py --full --cpu-seconds 0 --no-latency --sub-plans $k > "$OUT/k$k.json" 2> "$OUT/k$k.err"
  python -c "import json; d=json.load(open('$OUT/k$k.json')); print($k, d['value'], d['roofline']['avg_launch_ms'], d['roofline']['launches_timed'])"
done
