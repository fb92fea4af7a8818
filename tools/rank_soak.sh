# Six self-launched two-rank rehearsals of bench.py (gloo, both ranks on the one GPU),
# printing each line's rank verification; stops at the first failing run.
# usage: tools/rank_soak.sh [output directory]   (default: a fresh temporary directory)
set -u
cd "$(dirname "$0")/.."
OUT=${1:-$(mktemp -d)}
mkdir -p "$OUT"
echo "logs in $OUT"
for i in 1 2 3 4 5 6; do
  TTGA_BENCH_BACKEND=gloo timeout -k 10 240 python -u bench.py --full --gpus 2 --steps 10 --warmup 2 --no-pmc --no-cpu > "$OUT/self2_$i.log" 2> "$OUT/self2_$i.err" || { echo "run $i rc=$?"; exit 1; }
  python -c "
import json,sys
l=[x for x in open('$OUT/self2_$i.log') if x.startswith('{')][-1]
d=json.loads(l); r=d['ranks']; print($i, r['ranks_verified'], r['world'], [x.get('mismatch') for x in r['devices']])"
done
