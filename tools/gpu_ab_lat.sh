# B=1 latency (+ kernel stats) and the full C2 bench line on the current tree; output under $OUT (default ab_out/)
set -o pipefail
export TMPDIR=/tmp
T=${TAG:-ab}
O=${OUT:-ab_out}
mkdir -p $O
timeout -k 10 120 python tools/latency_b1.py > $O/${T}_lat.log 2>&1 && tail -1 $O/${T}_lat.log || exit 1
timeout -k 10 180 rocprofv3 --kernel-trace --stats --output-format csv -d $O/${T}_prof -o run -- python3 tools/latency_b1.py > $O/${T}_prof.log 2>&1 || exit 1
timeout -k 10 300 python bench.py --full --steps 20 --warmup 3 --traffic off --cpu-baseline off > $O/${T}_bench.log 2>&1 || exit 1
grep '^{' $O/${T}_bench.log | python -c "import json,sys; d=json.loads(sys.stdin.readline()); print('bench', d['value'], d['roofline']['kernel_ms'], d['roofline']['frac'], d['latency_b1_ms'], d['latency_b1_graph_ms'])"
