set -e
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$R/prof_out}; mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats -d $OUT/prof_r02c -o r02c --output-format csv -- python $R/bench.py --steps 2 --warmup 1 --full --no-cpu-baseline > $OUT/r02c_bench_under_rocprof.json 2> $OUT/r02c.err
KT=$(find $OUT/prof_r02c -name "*kernel_trace.csv")
python $R/tools/trace_tail.py $KT 0.12 > $OUT/r02c_trace_tail_steady_state.txt
python $R/tools/bond_timeline.py $KT 40 > $OUT/r02c_bond_timeline.txt
rm -f $KT
echo trace done
rocprofv3 --pmc FETCH_SIZE --kernel-include-regex "k_grouped_gemm_z" -d $OUT/pmc_r02_fetch -o f --output-format csv -- python $R/bench.py --steps 1 --warmup 1 --no-cpu-baseline > /dev/null 2> $OUT/pmc1.err
python $R/tools/pmc_summary.py $(find $OUT/pmc_r02_fetch -name "*counter_collection.csv") FETCH_SIZE 0.1 > $OUT/r02_pmc_gemm.txt
rm -rf $OUT/pmc_r02_fetch
echo fetch done
rocprofv3 --pmc WRITE_SIZE --kernel-include-regex "k_grouped_gemm_z" -d $OUT/pmc_r02_write -o w --output-format csv -- python $R/bench.py --steps 1 --warmup 1 --no-cpu-baseline > /dev/null 2> $OUT/pmc2.err
python $R/tools/pmc_summary.py $(find $OUT/pmc_r02_write -name "*counter_collection.csv") WRITE_SIZE 0.1 >> $OUT/r02_pmc_gemm.txt
rm -rf $OUT/pmc_r02_write
echo write done
rocprofv3 --pmc SQ_BUSY_CU_CYCLES SQ_VALU_MFMA_BUSY_CYCLES SQ_WAVES -d $OUT/pmc_r02_sq -o s --output-format csv -- python $R/bench.py --steps 1 --warmup 1 --no-cpu-baseline > /dev/null 2> $OUT/pmc3.err
python $R/tools/pmc_by_kernel.py $(find $OUT/pmc_r02_sq -name "*counter_collection.csv") 0.1 > $OUT/r02_pmc_sq_by_kernel.txt
rm -rf $OUT/pmc_r02_sq
echo sq done
