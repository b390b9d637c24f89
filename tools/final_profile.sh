# End-of-round evidence on the GPU box (from the repo root): bash tools/final_profile.sh <tag>; results in $OUT (default bench_out/)
#   $OUT/<tag>_bench.json                        `python bench.py --full` (un-profiled)
#   $OUT/<tag>_trace/...                         rocprofv3 --kernel-trace --stats of `python3 bench.py --full --no-cpu --steps 3 --repeats 2`
#   $OUT/<tag>_bench_2048frame_launches.txt      per-launch durations of the 2048-frame launches of that trace
#   gpurun_out/pmc_<tag>/...                     four separate --pmc passes over the extractor alone (tools/pmc_extract.sh)
#   $OUT/<tag>_gpu_tests.log, $OUT/<tag>_fuzz.log
TAG=${1:-r03}
export TMPDIR=/tmp
OUT=${OUT:-bench_out}; mkdir -p "$OUT"
python bench.py --full --steps 20 --warmup 5 > "$OUT/${TAG}_bench.json" 2> "$OUT/${TAG}_bench.err" && echo "bench ok"
rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/${TAG}_trace" -- python3 bench.py --full --no-cpu --steps 3 --repeats 2 > "$OUT/${TAG}_bench_under_rocprof.json" 2> "$OUT/${TAG}_bench_under_rocprof.err" && echo "trace ok"
python3 tools/trace_stage_summary.py $(ls "$OUT"/${TAG}_trace/*/*kernel_trace.csv | tail -1) 2048 > "$OUT/${TAG}_bench_2048frame_launches.txt"
bash tools/pmc_extract.sh $TAG 256 > gpurun_out/${TAG}_pmc.log 2>&1 && python3 tools/pmc_to_bench_csv.py gpurun_out/pmc_$TAG 256 gpurun_out/$TAG >> gpurun_out/${TAG}_pmc.log 2>&1 && echo "pmc ok"
timeout -k 10 900 python -m pytest tests -m gpu -x -q > "$OUT/${TAG}_gpu_tests.log" 2>&1; tail -2 "$OUT/${TAG}_gpu_tests.log"
timeout -k 10 420 python tools/fuzz_parity.py 300 20261005 > "$OUT/${TAG}_fuzz.log" 2>&1; tail -1 "$OUT/${TAG}_fuzz.log"
