# one measurement pass on the GPU box: bench (+e2e), rocprofv3 kernel stats, PMC fetch/write passes, phase stamps
#   gpurun -- 'TAG=r01g bash tools/measure_round.sh'
set -e
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
o=${OUT:-measure_out}/${TAG:-r01}; mkdir -p $o
timeout -k 10 300 python bench.py --steps 3 --warmup 1 --full > $o/bench.json 2> $o/bench.err
tail -c 600 $o/bench.json
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $o/prof -o runc -- python3 bench.py --steps 3 --warmup 1 --full --no-cpu-baseline > $o/prof_bench.json 2> $o/prof.err
timeout -k 10 300 rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d $o/pmc_fetch -o runc -- python3 bench.py --steps 2 --warmup 1 --no-cpu-baseline > /dev/null 2> $o/pmc1.err
timeout -k 10 300 rocprofv3 --kernel-trace --pmc WRITE_SIZE --output-format csv -d $o/pmc_write -o runc -- python3 bench.py --steps 2 --warmup 1 --no-cpu-baseline > /dev/null 2> $o/pmc2.err
FPC_DECODE_STAMPS=1 timeout -k 10 300 python tools/stamp_probe.py 256 2>&1 | grep -v amdgpu.ids | tail -13 > $o/stamps.txt
timeout -k 10 300 python tools/voiced_probe.py 256 >> $o/stamps.txt 2>&1
ls $o/prof
