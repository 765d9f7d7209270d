# bench + rocprofv3 kernel stats of the same command (GPU box):  bash tools/bench_prof.sh <tag>
set -e
cd "$(dirname "$0")/.."
out=${OUT:-out}
tag=${1:-x}
mkdir -p $out
true
true
export TMPDIR=/tmp
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $out/prof_${tag} -o r -- python3 bench.py --full --steps 10 --warmup 2 --no-cpu-baseline --no-config4 > $out/bench_under_rocprof_${tag}.json 2> $out/prof_${tag}.log
find $out/prof_${tag} -name "*kernel_stats*" | head
find $out/prof_${tag} -name "*kernel_trace*" -delete
