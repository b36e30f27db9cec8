#!/bin/bash
# stage-1 executor: tests, bench both drivers, busy-time breakdown (run from the repo root).   bash tools/stage1_lab.sh
R=$(pwd); O=$R/${OUT_DIR:-bench_runs}/s1; mkdir -p $O; cd /tmp; export TMPDIR=/tmp
cd $R
timeout 900 python -m pytest tests/test_stage1.py tests/test_raster_parity.py -x -q 2>&1 | tail -25 > $O/tests.log
timeout 300 python bench.py --full --stage 1 --steps 200 --warmup 30 > $O/bench_engine.json 2> $O/bench_engine.err

cd /tmp
timeout 400 rocprofv3 --kernel-trace --output-format csv -d $O/trace -o t -- python $R/bench.py --stage 1 --steps 80 --warmup 20 > /dev/null 2>&1
cd $R
python tools/stage1_busy.py $(ls $O/trace/*/*kernel_trace.csv $O/trace/*kernel_trace.csv 2>/dev/null | head -1) 60 > $O/busy.txt 2>&1
rm -rf $O/trace
cat $O/tests.log; python -c "import json;d=json.load(open(\"$O/bench_engine.json\"));print(d[\"value\"],d[\"ms_per_step\"],{k:round(v[\"avg_us\"],1) for k,v in d[\"kernels\"].items()})"; tail -3 $O/bench_engine.err; cat $O/busy.txt
