# quick A/B helper (GPU box): selected parity tests + the headline record with its golden parity; usage: tools/ab_quick.sh <output dir>
O=${1:?usage: tools/ab_quick.sh <output dir>}
mkdir -p $O
timeout -k 10 300 python -m pytest tests -m gpu -q -x -k "baseline_config or full_size or alternative_kernel or shapes_up or warm or predictor or ragged" > $O/sel.log 2>&1; echo "rc $?"; tail -3 $O/sel.log
for i in 1 2; do timeout -k 10 100 python bench.py --full --no-cpu-baseline --no-secondary --steps 20 > $O/bench_$i.json 2>/dev/null; python -c "
import json; d=json.load(open('$O/bench_$i.json')); print('headline', d['value'], d['roofline']['kernel_ms'], d['parity']['ok'], d['mean_ipm_iterations'])"; done
