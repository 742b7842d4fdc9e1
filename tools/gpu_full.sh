# Round-end measurement on one MI355X: GPU parity tests, the default (C2) bench line with the
# CPU baseline and the image check (bench.py --full; after a FETCH_SIZE PMC pass whose traffic it
# reports), and a kernel-trace profile of the same workload.
# usage: OUT=<directory for logs and profiles> sh tools/gpu_full.sh
set -o pipefail
cd "$(dirname "$0")/.." || exit 1
ROOT=$PWD
export TMPDIR=/tmp
R=${ROUND:-r01}
D=${OUT:?set OUT to the directory for logs and profiles}/full
mkdir -p $D
case $D in /*) ;; *) D=$ROOT/$D ;; esac
rm -f $D/parity_l2.jsonl
GI_PARITY_LOG=$D/parity_l2.jsonl timeout -k 10 900 python -u -m pytest ${PYTEST_TARGET:-tests} -x -v --durations=10 -m gpu -p no:cacheprovider --timeout 300 --timeout-method thread > $D/pytest_gpu.log 2>&1 || { tail -30 $D/pytest_gpu.log; exit 1; }
tail -2 $D/pytest_gpu.log
# FETCH_SIZE pass first, so the bench line below carries roofline.traffic from it
timeout -k 10 900 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $D/pmc -o run -- python3 bench.py --steps 1 --warmup 0 ${BENCH_ARGS:-} > $D/pmc.log 2>&1 || { tail -20 $D/pmc.log; exit 1; }
python3 tools/pmc_traffic.py $D/pmc/run_counter_collection.csv "${ROOF_KERNELS:-knn_chunk_lane_kernel,knn_lane_kernel}" 1024 2 1000000 1000000 $D/pmc.log > $D/traffic.log 2>&1 || { tail -5 $D/traffic.log; exit 1; }
timeout -k 10 900 python bench.py --full ${BENCH_ARGS:-} > $D/bench.log 2>&1 || { tail -20 $D/bench.log; exit 1; }
tail -1 $D/bench.log
timeout -k 10 900 rocprofv3 --kernel-trace --stats --output-format csv -d $D/trace -o run -- python3 bench.py --steps 1 --warmup 1 ${BENCH_ARGS:-} > $D/trace.log 2>&1 || { tail -20 $D/trace.log; exit 1; }
tail -1 $D/trace.log
cp profiles/knn_traffic.json $D/ 2>/dev/null || true
echo ok
