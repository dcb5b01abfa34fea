# the default bench with its roofline and extras (--full) three times in a row:  bash tools/bench_repeat.sh [outdir]
OUT=${1:-$(mktemp -d)}
mkdir -p "$OUT"
for k in 1 2 3; do
  timeout -k 10 600 python bench.py --full --no-cpu-baseline > "$OUT/bench_try$k.json" 2> /dev/null
  python tools/bench_line.py "$OUT/bench_try$k.json"
done
