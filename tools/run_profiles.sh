#!/bin/bash
# End-of-session evidence: bench record, rocprofv3 kernel-trace stats of the ONE-STREAM front-end bench (the headline
# configuration, no BA / CPU / pipelined legs in the traced process: the batched LocalBA leg crashed rocprofv3 in round 2), of
# the LocalBA batch and of GlobalBA at C5 size, API latencies, the RCCL world-size-1 run, the 2-rank shared-GPU dry run, the PMC
# passes.  Everything lands under gpurun_out/<round>/ ; tools/collect_profiles.py <round> copies what is judged into profiles/.
# usage: bash tools/run_profiles.sh r04 [quick]   (every leg is wrapped in `timeout`: a hung leg costs its limit, not the GPU budget)
cd "$(dirname "$0")/.."
export TMPDIR=/tmp
R=${1:-r06}
O=gpurun_out/$R; mkdir -p $O
step() { echo "== $*"; }
step bench;      timeout 900 python bench.py --full > $O/bench.json 2> $O/bench.err || tail -5 $O/bench.err
step bench trace
rm -rf $O/benchprof
rocprofv3 --kernel-trace --stats --output-format rocpd -d $O/benchprof -o run -- timeout 600 python bench.py --full --no-cpu --no-ba --no-pcie --streams 1 --no-pipelined --steps 3 --warmup 1 > $O/bench_traced.json 2> $O/benchprof.log || tail -5 $O/benchprof.log
db=$(find $O/benchprof -name "*.db" 2>/dev/null | head -1)
if [ -n "$db" ]; then python tools/rocpd_stats.py $db $O/bench_kernel_stats.csv && python tools/kstats_print.py $O/bench_kernel_stats.csv | head -14; else echo "no trace database"; fi
[ "$2" = quick ] && exit 0
step localba trace
rm -rf $O/lbaprof
rocprofv3 --kernel-trace --stats --output-format rocpd -d $O/lbaprof -o run -- timeout 600 python tools/ba_batch_thr.py 64:1 > $O/lbaprof.log 2>&1 || tail -5 $O/lbaprof.log
db=$(find $O/lbaprof -name "*.db" 2>/dev/null | head -1)
[ -n "$db" ] && python tools/rocpd_stats.py $db $O/localba_batch64_kernel_stats.csv && python tools/kstats_print.py $O/localba_batch64_kernel_stats.csv | head -14
timeout 600 python tools/ba_batch_thr.py 64:12:8 64:8:8 64:12:2 16:8:8 64:1:4 > $O/localba_throughput.txt 2>&1; cat $O/localba_throughput.txt
step localba trace, covisibility-structured and dense reduced systems
for st in covis dense; do
  rm -rf $O/lbaprof_$st
  ORBHIP_BENCH_STRUCTURE=$st rocprofv3 --kernel-trace --stats --output-format rocpd -d $O/lbaprof_$st -o run -- timeout 600 python tools/ba_batch_thr.py 64:1 > $O/lbaprof_$st.log 2>&1 || tail -5 $O/lbaprof_$st.log
  db=$(find $O/lbaprof_$st -name "*.db" 2>/dev/null | head -1)
  [ -n "$db" ] && python tools/rocpd_stats.py $db $O/localba_batch64_${st}_kernel_stats.csv && python tools/kstats_print.py $O/localba_batch64_${st}_kernel_stats.csv | head -6
  rm -rf $O/lbaprof_$st
done
step 12 callers: kernel trace, concurrency
rm -rf $O/lba12
rocprofv3 --kernel-trace --output-format rocpd -d $O/lba12 -o run -- timeout 600 python tools/ba_batch_thr.py 64:12:6 > $O/lba12.log 2>&1 || tail -5 $O/lba12.log
db=$(find $O/lba12 -name "*.db" 2>/dev/null | head -1)
[ -n "$db" ] && { grep solves $O/lba12.log; python tools/trace_overlap.py $db 0.5 0.9; } > $O/localba_trace_overlap_12_callers.txt 2>&1; cat $O/localba_trace_overlap_12_callers.txt
rm -rf $O/lba12
step ba pmc
timeout 900 bash tools/run_ba_pmc.sh $R 2>&1 | tail -18
step pt fuse a/b
timeout 600 python tools/pt_fuse_ab.py > $O/pt_fuse_ab.txt 2>&1; cat $O/pt_fuse_ab.txt
[ -f tools/scratch/lib_prof/liborbslam_hip.so ] && { step chol_wg phase stamps; timeout 300 python tools/chol_wg_prof.py 2>/dev/null | grep -v amdgpu.ids > $O/chol_wg_phase_prof.txt; cat $O/chol_wg_phase_prof.txt; }
[ -f tools/exp_lib/liborbslam_hip_sprof.so ] && { step schur phase stamps; timeout 300 python tools/schur_prof.py > $O/schur_phase_prof.txt 2>&1; cat $O/schur_phase_prof.txt; }
step diagonal factor: 1 / 2 / 4 waves, f64 latency table
REBUILD=1 timeout 600 python tools/factor_ab.py 2>/dev/null | grep -v "warning\|note:" > $O/factor_ab.txt; tail -5 $O/factor_ab.txt
[ -x tools/ubench/f64_latency ] && timeout 120 tools/ubench/f64_latency > $O/f64_latency.txt 2>&1; tail -3 $O/f64_latency.txt
[ -f tools/scratch/lib_prof/liborbslam_hip.so ] && { step chain phase stamps; timeout 300 python tools/chol_persist_prof.py > /dev/null 2>&1; cp gpurun_out/cholprof/chol_persist_prof.json $O/chol_persist_chain_c4.json; timeout 300 python tools/chol_persist_prof.py c5 > /dev/null 2>&1; cp gpurun_out/cholprof/chol_persist_prof_c5.json $O/chol_persist_chain_c5.json; }
step gba c5 trace
rm -rf $O/gbaprof
rocprofv3 --kernel-trace --stats --output-format rocpd -d $O/gbaprof -o run -- timeout 600 python tools/gba_c5_check.py 10 > $O/gbaprof.log 2>&1 || tail -5 $O/gbaprof.log
db=$(find $O/gbaprof -name "*.db" 2>/dev/null | head -1)
[ -n "$db" ] && python tools/rocpd_stats.py $db $O/gba_c5_kernel_stats.csv && python tools/kstats_print.py $O/gba_c5_kernel_stats.csv | head -12
step api latency
g++ -O2 -std=c++17 -I include tools/cpp/api_latency.cpp -o /tmp/api_latency -L ceres_mono_orb_slam2_amd/lib -lorbslam_hip && \
LD_LIBRARY_PATH=ceres_mono_orb_slam2_amd/lib:/opt/rocm/lib /tmp/api_latency > $O/api_latency_cpp.json; cat $O/api_latency_cpp.json
timeout 600 python tools/api_latency.py 2>/dev/null | tail -1 > $O/api_latency_py.json; cat $O/api_latency_py.json
step tracking latency
ORBHIP_TRACK_TIMING=1 timeout 300 python tools/track_latency.py 400 > $O/track_latency.txt 2>&1; tail -4 $O/track_latency.txt
step concurrency
timeout 600 python -m pytest tests/test_gpu_concurrency.py -q -s 2>&1 | grep -E "Tracking|passed|failed" > $O/concurrency.txt; cat $O/concurrency.txt
step mfma ubench
[ -x tools/ubench/bin/mfma_f64 ] && timeout 120 tools/ubench/bin/mfma_f64 > $O/mfma_f64_ubench.txt 2>&1; tail -4 $O/mfma_f64_ubench.txt
step rccl world size 1
ORBHIP_BENCH_FORCE_DIST=1 timeout 600 python -m torch.distributed.run --nnodes=1 --nproc-per-node 1 --master-addr 127.0.0.1 --master-port 29541 bench.py --gpus 1 --steps 3 --warmup 1 --no-cpu --no-pipelined --full > $O/bench_rccl_ws1.json 2> $O/bench_rccl_ws1.err || tail -5 $O/bench_rccl_ws1.err
step 2 ranks shared gpu
ORBHIP_BENCH_SHARED_GPU=1 timeout 900 python bench.py --gpus 2 --steps 5 --warmup 2 --no-cpu --full > $O/bench_2rank_shared.json 2> $O/bench_2rank.err || tail -5 $O/bench_2rank.err
# (the 8-rank run sharing ONE GPU is not part of this script since round 6: eight processes x 8 - 12 hardware queues x persistent, flag-linked
# launches oversubscribe the device - the run produced nothing twice and, run alone with a 1200-s limit, hit it and left the GPU
# unresponsive.  The N = 8 code path is the N = 2 one: tests/test_sharding*.py on gloo, the 2-rank run above, the RCCL run at world size 1.
# Do NOT run `ORBHIP_BENCH_SHARED_GPU=1 python bench.py --gpus 8` on a box you need afterwards.)
step fast phase profile
timeout 600 python tools/fast_phase_prof.py 2>/dev/null | python -c "import sys,json; t=sys.stdin.read(); i=t.index('{'); print(json.dumps(json.loads(t[i:])))" > $O/fast_phase_prof.json; cat $O/fast_phase_prof.json
step pmc
timeout 1200 bash tools/run_pmc.sh > $O/pmc.log 2>&1 || tail -5 $O/pmc.log
step mfma pmc
timeout 1100 bash tools/run_mfma_pmc.sh $R > $O/mfma_pmc.log 2>&1 || tail -5 $O/mfma_pmc.log
step collect
# the raw rocpd databases (PMC passes ~50 MB, traces) exceed what gpurun copies back: collect on the box, keep the summaries only
PROFILES_OUT=$PWD/$O/collected python tools/collect_profiles.py $R | tail -30
rm -rf gpurun_out/pmc_x_insts gpurun_out/pmc_x_active gpurun_out/pmc_x_fetch gpurun_out/pmc_x_write $O/benchprof $O/lbaprof $O/gbaprof
du -sh gpurun_out
