# the round-end sequence on the GPU box (GPU tests, smoke, the full bench line): tools/dev/final_check.sh <tag> <output dir>
T=${1:-last}
O=${2:?usage: tools/dev/final_check.sh <tag> <output dir>}
mkdir -p $O
timeout -k 10 600 python -m pytest tests -m gpu -x -q > $O/gputests_$T.log 2>&1; tail -2 $O/gputests_$T.log \
 && python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" \
 && python bench.py --gpus 1 --steps 20 --warmup 5 --full > $O/bench_$T.json 2> $O/bench_$T.err \
 && python -c "
import json; d=json.loads(open('$O/bench_$T.json').read().strip().splitlines()[-1])
print(d['value'], d['ms_per_step'], d['roofline']['kernel_ms'], all(s['parity']['ok'] for s in d['secondary']))"
