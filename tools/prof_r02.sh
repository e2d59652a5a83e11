# Round-2 profiling passes (one gpurun call): the stage-1 step (metric 2) and the config-1 interpolator loop (metric 1).
# PMC passes are separate runs without any trace domain, as the pool requires.
set -e
R=$GRAFT_REPO_ROOT; O=$R/gpurun_out/prof_r02; rm -rf $O; mkdir -p $O
cd /tmp && export TMPDIR=/tmp
export AFI_BENCH_OTHER_DTYPES=0      # the profiled runs hold the default arithmetic only (the default run at the end reports every setting)
B="python3 $R/bench.py --full"
L="python3 $R/tools/cfg1_loop.py"
SQ="SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_VALU_MFMA_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE"
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/trace -o step -- $B --steps 3 --warmup 0 --no-interp --no-cpu-baseline > $O/bench_trace.log 2>&1
echo step trace done
timeout -k 10 300 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $O/pmc_fetch -o step -- $B --steps 1 --warmup 0 --no-interp --no-cpu-baseline > $O/bench_fetch.log 2>&1
timeout -k 10 300 rocprofv3 --pmc WRITE_SIZE --output-format csv -d $O/pmc_write -o step -- $B --steps 1 --warmup 0 --no-interp --no-cpu-baseline > $O/bench_write.log 2>&1
timeout -k 10 300 rocprofv3 --pmc $SQ --output-format csv -d $O/pmc_sq -o step -- $B --steps 1 --warmup 0 --no-interp --no-cpu-baseline > $O/bench_sq.log 2>&1
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/trace_fp32 -o step -- $B --steps 3 --warmup 0 --no-interp --no-cpu-baseline --dtype fp32 > $O/bench_trace_fp32.log 2>&1
export AFI_D_OVERLAP=0      # the dominant kernel with the chip to itself (the default step runs the D phase on two streams)
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/trace_serial -o step -- $B --steps 3 --warmup 0 --no-interp --no-cpu-baseline > $O/bench_trace_serial.log 2>&1
timeout -k 10 300 rocprofv3 --pmc $SQ --output-format csv -d $O/pmc_sq_serial -o step -- $B --steps 1 --warmup 0 --no-interp --no-cpu-baseline > $O/bench_sq_serial.log 2>&1
unset AFI_D_OVERLAP
echo step pmc done
timeout -k 10 200 rocprofv3 --kernel-trace --stats --output-format csv -d $O/cfg1_trace -o cfg1 -- $L 100 > $O/cfg1_trace.log 2>&1
timeout -k 10 200 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $O/cfg1_fetch -o cfg1 -- $L 20 > $O/cfg1_fetch.log 2>&1
timeout -k 10 200 rocprofv3 --pmc WRITE_SIZE --output-format csv -d $O/cfg1_write -o cfg1 -- $L 20 > $O/cfg1_write.log 2>&1
timeout -k 10 200 rocprofv3 --pmc $SQ --output-format csv -d $O/cfg1_sq -o cfg1 -- $L 20 > $O/cfg1_sq.log 2>&1
echo cfg1 passes done
unset AFI_BENCH_OTHER_DTYPES
cd $R && timeout -k 10 200 $L 200 g > $O/cfg1_default.log 2>&1
cd $R && timeout -k 10 500 python bench.py --full > $O/bench_default.log 2> $O/bench_default.err
echo default done
find $O -name "*.csv" | head -40
