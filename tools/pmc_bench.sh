#!/bin/bash
# Round profile set for the default bench (run on the GPU box through gpurun, from the repo root):  tools/pmc_bench.sh r02
#   profiles/<tag>_pmc_summary.json          three separate --pmc passes (FETCH_SIZE | WRITE_SIZE | MFMA busy), done FIRST so
#                                            that the bench lines below carry the fresh `traffic`
#   profiles/<tag>_bench.json                python bench.py --full
#   profiles/<tag>_bench_kernel_stats.csv    rocprofv3 --kernel-trace --stats of the same command
#   profiles/<tag>_bench_under_rocprof.json  bench line of that profiled run
tag=${1:-r02}
R=$PWD
OUT=${OUT:-$R/bench_out}          # raw outputs (profiler directories, bench lines); profiles/ gets the summary
mkdir -p $OUT $R/profiles
cd /tmp && export TMPDIR=/tmp
rm -rf $OUT/prof_stats $OUT/pmc
# one stream, no extras: per-kernel averages of the headline configuration only (the bench line's own roofline pass is single-stream too)
CMD="python $R/bench.py --steps 3 --warmup 1 --streams 1 --no-cpu-baseline --no-roofline --no-extras"
rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d $OUT/pmc/fetch -o p -- $CMD > /dev/null 2>&1
rocprofv3 --kernel-trace --pmc WRITE_SIZE --output-format csv -d $OUT/pmc/write -o p -- $CMD > /dev/null 2>&1
rocprofv3 --kernel-trace --pmc SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE SQ_WAVES --output-format csv -d $OUT/pmc/mfma -o p -- $CMD > /dev/null 2>&1
cd $R
python tools/pmc_summary.py $OUT/pmc $OUT/${tag}_pmc_summary.json > /dev/null
cp $OUT/${tag}_pmc_summary.json profiles/${tag}_pmc_summary.json
python bench.py --full > $OUT/${tag}_bench.json 2> $OUT/${tag}_bench.err
cd /tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_stats -- python $R/bench.py --full --streams 1 --no-cpu-baseline --no-extras > $OUT/${tag}_bench_under_rocprof.json 2>/dev/null
cp $(ls $OUT/prof_stats/*/*kernel_stats.csv | head -1) $OUT/${tag}_bench_kernel_stats.csv
cd $R
python tools/prof_summary.py $OUT/${tag}_bench_kernel_stats.csv $OUT/${tag}_bench_under_rocprof.json auto 48
python - <<PY
import json
d = json.load(open("$OUT/${tag}_bench.json")); r = d["roofline"]
print("bench: %.1f frames/s, %.2f ms/step; dominant %s: %.1f TF = %.3f of %.0f, launch %.1f us, traffic %s; path_hbm_frac %.3f" %
      (d["value"], d["ms_per_step"], r["kernel"], r["achieved"], r["frac"], r["peak"], r["avg_launch_us"], r["traffic"], r.get("path_hbm_frac", -1)))
print("cpu_baseline", d.get("cpu_baseline"))
PY
# variants quoted in DESIGN.md §5 (one bench line each; no CPU baseline, no roofline pass)
if [ "${2:-}" = "variants" ]; then
  for v in "bf16x3:--conv-math bf16x3" "f32:--conv-math f32" "streams1:--streams 1" "streams3:--streams 3" "device_results:--device-results" "1frame:--frames 1 --steps 100 --streams 1" "4frames:--frames 4 --steps 100 --streams 1" "4frames_2streams:--frames 4 --steps 100" "16frames:--frames 16 --steps 48" "canonical_rows:--row-order canonical" "fp32_dense_maps:--dense-pairs 0" "modules:--api modules"; do
    python bench.py --no-cpu-baseline --no-roofline --no-extras ${v#*:} > $OUT/${tag}_bench_${v%%:*}.json 2>> $OUT/${tag}_bench.err
    python -c "import json,sys; d=json.load(open('$OUT/${tag}_bench_${v%%:*}.json')); print('${v%%:*}', round(d['value'],1), 'frames/s', round(d['ms_per_step'],2), 'ms/step')"
  done
  python bench.py --full --mode train --steps 40 --warmup 10 > $OUT/${tag}_train_bench.json 2>> $OUT/${tag}_bench.err
  python -c "import json; d=json.load(open('$OUT/${tag}_train_bench.json')); print('train', round(d['value'],1), 'frames/s', round(d['ms_per_step'],2), 'ms/step')"
  cd /tmp
  rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_train -- python $R/bench.py --full --mode train --steps 40 --warmup 10 > $OUT/${tag}_train_bench_under_rocprof.json 2>/dev/null
  cp $(ls $OUT/prof_train/*/*kernel_stats.csv | head -1) $OUT/${tag}_train_kernel_stats.csv
  cd $R
fi
