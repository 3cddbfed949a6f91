#!/bin/bash
# Inference bench (default config) per-layer table + rocprofv3 kernel stats.
OUT=${OUT:-$PWD/bench_out}
mkdir -p $OUT
python bench.py --full --no-cpu-baseline --layers > $OUT/infer_bench.json 2> $OUT/infer_layers.txt
cat $OUT/infer_layers.txt | grep -v Warn
python -c "
import json; d=json.load(open('$OUT/infer_bench.json')); r=d['roofline']
print(d['value'], d['ms_per_step'], r['kernel'], r['achieved'], r['avg_launch_us'], r['chip_conv_tflops'])
for k,v in r['all_conv_kernels'].items(): print(k, v)
"
R=$PWD
cd /tmp && export TMPDIR=/tmp
rm -rf $OUT/infer_prof
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/infer_prof -- python $R/bench.py --full --no-cpu-baseline --no-roofline > /dev/null 2>&1
cd $R
f=$(ls $OUT/infer_prof/*/*kernel_stats.csv | head -1)
cp $f $OUT/infer_kernel_stats.csv
python - "$f" <<'PY'
import csv, sys
rows = list(csv.DictReader(open(sys.argv[1])))
tot = sum(float(r["TotalDurationNs"]) for r in rows)
nf = 20 * 8
print("total kernel ms / frame: %.3f" % (tot / nf / 1e6))
for r in rows[:30]:
    print("%-60s calls %5s  avg %9.1f us  %5.1f%%  us/frame %.1f" % (r["Name"][:60], r["Calls"], float(r["AverageNs"]) / 1e3,
          float(r["Percentage"]), float(r["TotalDurationNs"]) / nf / 1e3))
PY
