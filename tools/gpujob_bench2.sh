# Round-2 bench: default config-B line (with CPU baseline), config C at N=1,
# rocprofv3 kernel stats of the default command.  Results go to $OUT (bench_out/).
set -o pipefail
TAG=${TAG:-r02}
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
OUT=${OUT:-bench_out}
mkdir -p $OUT/profiles_new
timeout -k 10 600 python3 bench.py --full > $OUT/bench_$TAG.json 2> $OUT/bench_$TAG.err || { tail -20 $OUT/bench_$TAG.err; exit 14; }
cat $OUT/bench_$TAG.json
timeout -k 10 300 python3 bench.py --config C --steps 1 --warmup 1 > $OUT/benchC_$TAG.json 2> $OUT/benchC_$TAG.err || { tail -20 $OUT/benchC_$TAG.err; exit 16; }
cat $OUT/benchC_$TAG.json
if [ -z "$NOPROF" ]; then
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_bench -o run -- python3 bench.py --steps 1 --warmup 1 > $OUT/prof_bench.log 2>&1 || { tail -20 $OUT/prof_bench.log; exit 15; }
S=$(find $OUT/prof_bench -name "*kernel_stats.csv" | head -1); cp $S $OUT/profiles_new/${TAG}_bench_kernel_stats.csv; head -14 $S
fi
echo done
