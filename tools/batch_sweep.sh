# C2 against the per-GPU batch: clips/s, ms per step and the roofline leg's TFLOP/s.  usage: bash tools/batch_sweep.sh OUT_DIR
OUT="${1:?usage: bash tools/batch_sweep.sh OUT_DIR}"
mkdir -p "$OUT"
for b in 8 16 32 64 128; do
  python bench.py --full --no-cpu-baseline --batch $b --steps 10 2>/dev/null > "$OUT/sweep_$b.json"
  python -c "import json, sys; d=json.load(open(sys.argv[1])); print('B', $b, d['value'], d['ms_per_step'], d['roofline']['achieved'])" "$OUT/sweep_$b.json"
done
