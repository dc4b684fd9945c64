# Full validation on one MI355X box: every GPU test, smoke(), then bench.py --full at configs 2, 4, 5, 1, cad1 and a2
# (logs and JSON lines under $OUT, default full_out/); stops at the first failure.
# usage: [OUT=dir] bash tools/gpu_full.sh TAG
set -o pipefail
TAG=${1:-r05}
OUT=${OUT:-full_out}
mkdir -p $OUT
timeout -k 10 600 python -u -m pytest tests -m gpu -x -v --timeout 300 --timeout-method thread > $OUT/${TAG}_gputest_full.log 2>&1 && \
timeout -k 10 120 python -u -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > $OUT/${TAG}_smoke.log 2>&1 && \
timeout -k 10 300 python bench.py --full > $OUT/${TAG}_bench_cfg2_full.json 2> $OUT/${TAG}_bench_cfg2.err && \
timeout -k 10 300 python bench.py --full --config 4 > $OUT/${TAG}_bench_cfg4.json 2> $OUT/${TAG}_bench_cfg4.err && \
timeout -k 10 300 python bench.py --full --config 5 > $OUT/${TAG}_bench_cfg5.json 2> $OUT/${TAG}_bench_cfg5.err && \
timeout -k 10 300 python bench.py --full --config 1 > $OUT/${TAG}_bench_cfg1.json 2> $OUT/${TAG}_bench_cfg1.err && \
timeout -k 10 300 python bench.py --full --config cad1 > $OUT/${TAG}_bench_cad1.json 2> $OUT/${TAG}_bench_cad1.err && \
timeout -k 10 300 python bench.py --full --config a2 > $OUT/${TAG}_bench_a2.json 2> $OUT/${TAG}_bench_a2.err
