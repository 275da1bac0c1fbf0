#!/bin/bash
# Sample rocm-smi while the bench loops (GPU box only).
cd "$(dirname "$0")/.."
LOG=$(mktemp)
python bench.py --full --steps 2000 --warmup 3 --no-cpu-baseline > "$LOG" 2>&1 &
BP=$!
sleep 6
for i in 1 2 3; do
  rocm-smi --showpower --showclocks --showtemp 2>&1 | grep -E "Power|sclk|mclk|fclk|Temperature \(Sensor (junction|memory)" | head -12
  echo ---
  sleep 1
done
wait $BP
tail -1 "$LOG" | cut -c1-200
rm -f "$LOG"
