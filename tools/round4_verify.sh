# GPU-box verification: the whole -m gpu suite, the bench lines of every configuration, rocprofv3 summaries + PMC traffic of the
# default command (both maths), the half-mode line and profile, the upload-inclusive A/B of the schedules: tools/round4_verify.sh OUTDIR
O=${1:?usage: tools/round4_verify.sh OUTDIR}; mkdir -p $O
python -m pytest tests -m gpu -x -q > $O/verify_tests.log 2>&1; grep -E "passed|failed" $O/verify_tests.log | tail -2
python bench.py --full > $O/bench_default.json 2> $O/bench_default.err; tail -c 200 $O/bench_default.json; echo
for c in cfg3 cfg5; do python bench.py --full --config $c > $O/bench_$c.json 2> $O/bench_$c.err; done
python bench.py --full --half --no-extras --cpu-frames 0 --latency-steps 0 > $O/bench_half.json 2> $O/bench_half.err
YDS_HALF_H16=1 python bench.py --full --half --no-extras --cpu-frames 0 --latency-steps 0 > $O/bench_half_h16.json 2> $O/bench_half_h16.err
python bench.py --full --half --config cfg3 --no-extras --cpu-frames 0 --latency-steps 0 > $O/bench_half_cfg3.json 2> $O/bench_half_cfg3.err
PMC=1 bash tools/profile_bench.sh cfg2 $O/prof_cfg2 > $O/prof_cfg2.log 2>&1
MATH=f32 PMC=1 bash tools/profile_bench.sh cfg2 $O/prof_cfg2_f32 > $O/prof_cfg2_f32.log 2>&1
bash tools/profile_bench.sh cfg3 $O/prof_cfg3 > $O/prof_cfg3.log 2>&1
bash tools/profile_bench.sh cfg5 $O/prof_cfg5 > $O/prof_cfg5.log 2>&1
HALF=1 bash tools/profile_bench.sh cfg2 $O/prof_half > $O/prof_half.log 2>&1
for s in 0 -1 0 -1; do python tools/upload_prof.py --schedule $s; done 2>&1 | grep frames
