set -e
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$R/prof_out}; mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats -d $OUT/prof_r03c512 -o c512 --output-format csv -- python $R/bench.py --steps 2 --warmup 1 --full --no-cpu-baseline --chi 512 > $OUT/r03c512_bench.json 2> $OUT/r03c512.err
KT=$(find $OUT/prof_r03c512 -name "*kernel_trace.csv")
python $R/tools/trace_tail.py $KT 0.12 > $OUT/r03c512_trace_tail.txt
python $R/tools/bond_timeline.py $KT 40 > $OUT/r03c512_bond_timeline.txt
rm -f $KT
