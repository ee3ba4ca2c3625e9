#!/bin/bash
# tools/profile.sh <target> [args] -- the one entry point for measurements on the GPU box:
#   gpurun --timeout 900 -- 'bash tools/profile.sh <target>'
# Everything is written under gpurun_out/<round>/ (scratch; MXA_ROUND, default r06); what is worth keeping is copied to profiles/ by hand.
# Targets:
#   tests [pytest args]  all -m gpu tests + smoke(); full log in gputests_full.txt
#   bench [bench args]   bench.py --full line -> bench_n1.json (+ bench_detail.json)
#   stats                bench.py (headline only) under rocprofv3 --kernel-trace --stats -> bench_n1_kernel_stats.csv
#   pmc-mfma <gemm|i8|xprod_f4|xprod_i8>        SQ counter pass (MFMA busy, clock, waits) of one kernel family -> pmc_mfma_util_<t>.json
#   pmc-traffic <gemm|i8|gram|xprod_f4|xprod_i8>  FETCH_SIZE / WRITE_SIZE passes (separate runs) -> pmc_traffic_<t>.txt
#   harness [big]        the reference's benchmark.f90 (GPU mode, unmodified) with the phase clock of the plain ABI (PRINT_LEVEL=1)
#   power [seconds]      power + clock trace: bare MFMA loops (f4, i8, f64), k_gemm, k_crossprod_gang FP4 / int8 (tools/power_trace.py); PT_TARGETS="i8t1 i8tn1 gram hbm_plain hbm_tn": the
#                        int8 kernels of a CG step, the whole step, and their data movement alone
#   gram                 CG step (config-5 shard): step time + kernel timeline of three steps
#   xprod [snps indiv]   crossproduct kernel time at config 3, both engines
#   ld-band [snps indiv window]   windowed LD (mxa_ld_band / mxa_ld_scores): kernel time, tiles, bytes written, both engines; band vs full mxa_ld (A/B)
#   ld-pairwise [snps indiv window]   pairwise-complete windowed LD (mxa_ld_band_pairwise / mxa_ld_scores_pairwise) against mxa_ld_band / mxa_ld_scores, one process, both engines
#   ld-window-var [snps indiv window]   windowed LD over last[] (mxa_ld_window_rows / mxa_ld_window_scores) against mxa_ld_band / mxa_ld_scores, one process, both engines; a density profile
#   ld-pairs [snps indiv window min_r2]   pairs with r^2 >= min_r2 as CSR (mxa_ld_window_pairs / _pairwise) against mxa_ld_window_rows(_pairwise), one process, both engines
#   ld-prune [snps indiv window min_r2 reps]   LD pruning / clumping on the device (mxa_ld_window_prune, mxa_ld_prune_csr): products, select passes, rounds, owner pass; three priorities; against ld_pairs + the walk on the host
#   ld-apply [snps indiv window reps]   the window applied to a matrix (mxa_ld_window_apply), n in {1, 16, 64}, against mxa_ld_window_scores and against mxa_ld_window_rows + a device band product in torch, one process, both engines
#   ld-op [snps indiv window reps]   the LD operator object (mxa_ld_op_*): creation against mxa_ld_window_rows, apply at n in {1, 16, 64} against mxa_ld_window_apply with the byte model, a 50-iteration solve, one process
#   assoc [snps indiv reps]   the association scan (mxa_assoc_linear) at n = 1, k = 15 and n = 16, k = 16, without and with 5 % missing calls, against the bare 'T' product of n + k columns on a resident object, one process
#   assoc-kernels [snps indiv]   the library kernels inside mxa_assoc_linear, one by one: tools/perf_assoc.py ... trace under rocprofv3 --kernel-trace, in a run of its own
#   assoc-score [snps indiv reps]   the score test (mxa_assoc_score) at n = 1, q = 15 and n = 4, q = 15, without and with 5 % missing calls, beside mxa_assoc_linear at n = 1, k = 15 and the bare 'T' products of the same column counts, one process, alternating calls
#   assoc-score-kernels [snps indiv]   the library kernels inside mxa_assoc_score, one by one: tools/perf_assoc.py score ... trace under rocprofv3 --kernel-trace, in a run of its own
#   assoc-spa [snps indiv reps]   the score test with saddlepoint p-values (mxa_assoc_score_spa) at n = 1, q = 3, 5 % cases, z_cutoff = 1.96 and inf, beside mxa_assoc_score on the same operands, one process, alternating calls
#   assoc-spa-kernels [snps indiv]   the library kernels inside mxa_assoc_score_spa, one by one: tools/perf_assoc_spa.py ... trace under rocprofv3 --kernel-trace, in a run of its own
#   assoc-firth [snps indiv reps]   the score test with effect sizes (mxa_assoc_score_firth, penalty 0 and 1) at n = 1, q = 3, 5.5 % cases, z_cutoff = 1.96, beside mxa_assoc_score and mxa_assoc_score_spa on the same operands, one process, alternating calls
#   assoc-firth-kernels [snps indiv]   the library kernels inside mxa_assoc_score_spa and mxa_assoc_score_firth, one by one, with the time per item and per (item, evaluation) of k_assoc_spa and k_assoc_firth: tools/perf_assoc_firth.py ... trace under rocprofv3 --kernel-trace, in a run of its own
#   assoc-set [snps indiv reps]   the set tests (mxa_assoc_set) with sets of 32, 8 and 256 neighbouring SNPs at n = 1, q = 3, beside mxa_assoc_score on the same operands and beside the torch route (decode to fp64 + bmm), one process, alternating calls
#   assoc-set-kernels [snps indiv]   the library kernels inside mxa_assoc_set, one by one: tools/perf_assoc_set.py ... trace under rocprofv3 --kernel-trace, in a run of its own
#   assoc-mixed [snps indiv blocks]   the mixed-model scan (miraculix_amd.mixed.assoc_mixed) at n = 1, q = 3, LOCO over the blocks: one whole call, split into the kinship products, the score scan and everything else (HIP events), and the kernel classes of a run of its own under rocprofv3 --kernel-trace
#   gemm <snps indiv n reps>   k_gemm / k_gemm_i8 kernel time of one shape, 'N' and 'T'
#   rehearse             the driver's N > 1 bench commands on one GPU (8 virtual shards in-process; 2 and 4 launcher ranks over gloo)
#   soak                 tools/soak.py + fuzz_shapes.py + fuzz_crossprod.py
set -o pipefail
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}" || exit 1
R=$PWD
RND=${MXA_ROUND:-r06}
O=$R/gpurun_out/$RND; mkdir -p "$O"
export TMPDIR=/tmp
SQ="SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_VALU_MFMA_BUSY_CYCLES SQ_INSTS_VALU SQ_INSTS_LDS GRBM_GUI_ACTIVE"
T=$1; shift

# the program (after `--` of rocprofv3: python3 itself, never a wrapper) and the kernel-name filter of a kernel family
family() {
  case "$1" in
    gemm)     PROG="python3 $R/tools/perf_gemm.py 1000000 50000 32 2"; KERN="k_gemm<" ;;
    i8)       PROG="python3 $R/tools/perf_gemm.py 250000 100000 1 5"; KERN="k_gemm_i8" ;;
    gram)     PROG="python3 $R/tools/perf_gram.py 250000 100000 1"; KERN="mxa::" ;;
    xprod_f4) unset MXA_XPROD_ENGINE; PROG="python3 $R/tools/perf_crossprod.py 500000 100000 2"; KERN="k_crossprod_gang" ;;
    xprod_i8) export MXA_XPROD_ENGINE=i8; PROG="python3 $R/tools/perf_crossprod.py 500000 100000 2"; KERN="k_crossprod_gang" ;;
    *) echo "unknown kernel family $1"; exit 2 ;;
  esac
}

case "$T" in
tests)
  timeout -k 10 1100 python -m pytest tests -x -q -m gpu "$@" > "$O/gputests_full.txt" 2>&1; rc=$?
  tail -c 6000 "$O/gputests_full.txt"; tail -6 "$O/gputests_full.txt" > "$O/gputests.txt"; [ $rc = 0 ] &&
  timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -1 | tee -a "$O/gputests.txt" ;;
bench)
  timeout -k 10 1100 python bench.py --full "$@" > "$O/bench_n1.json" 2> "$O/bench_n1.stderr"; rc=$?
  cp -f bench_detail.json "$O/bench_detail.json" 2>/dev/null
  tail -c 4500 "$O/bench_n1.json"; tail -3 "$O/bench_n1.stderr"; exit $rc ;;
stats)
  rm -rf "$O/stats"
  ( cd /tmp && timeout -k 10 900 rocprofv3 --kernel-trace --stats --output-format csv -d "$O/stats" -- python3 "$R/bench.py" --no-pmc --no-configs --no-abi --no-alt-engine --no-cpu-baseline --steps 10 > "$O/stats_bench.json" 2> "$O/stats.stderr" ) || { tail -5 "$O/stats.stderr"; exit 1; }
  f=$(find "$O/stats" -name '*kernel_stats.csv' | head -1) && cp "$f" "$O/bench_n1_kernel_stats.csv" && head -8 "$f"; rm -rf "$O/stats" ;;
pmc-mfma)
  family "${1:-gemm}"; D="$O/pmc_$1"; rm -rf "$D"; mkdir -p "$D"
  ( cd /tmp && timeout -k 10 700 rocprofv3 --pmc $SQ --kernel-trace --output-format csv -d "$D" -- $PROG > "$D/run.log" 2>&1 ) || { tail -5 "$D/run.log"; exit 1; }
  tail -2 "$D/run.log"; python3 tools/pmc_mfma_util.py "$D" "$KERN" "$O/pmc_mfma_util_$1.json"; rm -rf "$D"/*/ ;;
pmc-traffic)
  family "${1:-gemm}"
  for c in FETCH_SIZE WRITE_SIZE; do
    D="$O/pmc_${1}_$c"; rm -rf "$D"; mkdir -p "$D"
    ( cd /tmp && timeout -k 10 700 rocprofv3 --pmc $c --kernel-trace --output-format csv -d "$D" -- $PROG > "$D/run.log" 2>&1 ) || { tail -5 "$D/run.log"; exit 1; }
  done
  python3 tools/pmc_traffic.py "$O/pmc_${1}_FETCH_SIZE" "$O/pmc_${1}_WRITE_SIZE" "$KERN" "$O/pmc_traffic_$1.json" 2>&1 | tee "$O/pmc_traffic_$1.txt"; rm -rf "$O"/pmc_${1}_*/*/ ;;
harness)
  D=/tmp/refdata; mkdir -p $D
  if [ "$1" = big ]; then S=250000; I=50000; else S=100000; I=20000; fi
  python3 tools/make_bed_dataset.py $D/d $S $I || exit 1
  for i in 1 2; do
    ( cd $D && PRINT_LEVEL=1 OMP_NUM_THREADS=16 timeout -k 10 500 "$R/oracle/_ref/fortran/benchmark.out" GPU d.bed d.freq > "$O/harness_${S}x${I}_run$i.txt" 2>&1 ) || exit 1
    grep -E "Elapsed time|Average time|dgemm_compressed '" "$O/harness_${S}x${I}_run$i.txt" | cut -c1-330 | head -50
  done
  rm -rf $D ;;
power)
  [ -x tools/mfma_power_probe ] || hipcc -O3 --offload-arch=gfx950 -o tools/mfma_power_probe tools/mfma_power_probe.hip || exit 1
  for t in ${PT_TARGETS:-bare_f4 bare_i8 bare_f64 gemm xprod_f4 xprod_i8}; do
    timeout -k 10 300 python3 tools/power_trace.py $t ${1:-12} > "$O/power_trace_$t.txt" 2>&1 || { tail -5 "$O/power_trace_$t.txt"; exit 1; }
    tail -1 "$O/power_trace_$t.txt"
  done ;;
gram)
  timeout -k 10 600 python3 tools/perf_gram.py 250000 100000 1 2>&1 | tee "$O/gram.txt" || exit 1
  D="$O/gram_trace"; rm -rf "$D"
  ( cd /tmp && timeout -k 10 600 rocprofv3 --kernel-trace --output-format csv -d "$D" -- python3 "$R/tools/perf_gram.py" 250000 100000 1 > "$O/gram_trace_run.log" 2>&1 ) || exit 1
  python3 - "$(find "$D" -name '*kernel_trace.csv' | head -1)" <<'PY' | tee "$O/gram_step_kernel_timeline.txt"
import csv, sys
rows = [r for r in csv.DictReader(open(sys.argv[1])) if "mxa::" in r["Kernel_Name"]]
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
tail = rows[-21:]
t0, prev = int(tail[0]["Start_Timestamp"]), None
for r in tail:
    s, e = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
    print(f"{(s - t0) / 1e3:9.1f} us  +{((s - prev) / 1e3 if prev else 0.0):6.1f} gap  {(e - s) / 1e3:8.1f} us  {r['Kernel_Name'].split('(')[0][:60]}")
    prev = e
PY
  rm -rf "$D" ;;
xprod)
  for e in f4 i8; do
    if [ $e = i8 ]; then export MXA_XPROD_ENGINE=i8; else unset MXA_XPROD_ENGINE; fi
    timeout -k 10 500 python3 tools/perf_crossprod.py ${1:-500000} ${2:-100000} 2 2>&1 | tee -a "$O/xprod.txt" || exit 1
  done ;;
ld-band)
  # band + scores at config 2's shape, both engines; then band against the full mxa_ld where the full result exists (100 000 SNPs: 80 GB), A/B alternating
  for e in f4 i8; do
    if [ $e = i8 ]; then export MXA_XPROD_ENGINE=i8; else unset MXA_XPROD_ENGINE; fi
    timeout -k 10 400 python3 tools/perf_ld_band.py ${1:-1000000} ${2:-50000} ${3:-1023} 5 2>&1 | tee -a "$O/ld_band.txt" || exit 1
  done
  unset MXA_XPROD_ENGINE
  timeout -k 10 400 python3 tools/perf_ld_band.py 100000 ${2:-50000} ${3:-1023} 5 --vs-full 2>&1 | tee -a "$O/ld_band.txt" || exit 1 ;;
ld-pairwise)
  # 5 % missing (six products per band tile) and the same genotypes without missing codes (fast path) against the plain entries, alternating calls
  timeout -k 10 500 python3 tools/perf_ld_pairwise.py ${1:-1000000} ${2:-50000} ${3:-1023} 5 2>&1 | tee -a "$O/ld_pairwise.txt" || exit 1 ;;
ld-window-var)
  # the general entries with last[i] = min(i + window, snps - 1) against the fixed ones (same tiles), then a density profile with the same mean reach, alternating calls
  timeout -k 10 500 python3 tools/perf_ld_window_var.py ${1:-1000000} ${2:-50000} ${3:-1023} 5 2>&1 | tee -a "$O/ld_window_var.txt" || exit 1 ;;
ld-pairs)
  # count-only and filling calls of the pairs entries against the rows entries over the same last[], plain and pairwise (5 % missing; no missing code: one product), alternating calls
  timeout -k 10 500 python3 tools/perf_ld_pairs.py ${1:-1000000} ${2:-50000} ${3:-1023} ${4:-0.2} 5 2>&1 | tee -a "$O/ld_pairs.txt" || exit 1 ;;
ld-prune)
  # data with LD structure; HIP events of the products + select passes, the rounds and the owner pass under a random priority, -MAF and NULL; the host route (ld_pairs + the sequential walk) beside it
  timeout -k 10 800 python3 tools/perf_ld_prune.py ${1:-1000000} ${2:-50000} ${3:-1023} ${4:-0.2} ${5:-5} 2>&1 | tee -a "$O/ld_prune.txt" || exit 1 ;;
ld-apply)
  # kernel and whole-call time of the apply entry per n and the two comparison legs, alternating calls; the text is what profiles/r13_ld_apply.txt holds
  timeout -k 10 900 python3 tools/perf_ld_apply.py ${1:-1000000} ${2:-50000} ${3:-1023} ${4:-5} 2>&1 | tee "$O/ld_apply.txt" || exit 1
  cp -f "$O/ld_apply.txt" "$R/profiles/r13_ld_apply.txt" ;;
ld-op)
  # whole-call times of creation, apply and solve against the entries that redo the products, alternating calls; the text is what profiles/r14_ld_op.txt holds
  timeout -k 10 900 python3 tools/perf_ld_op.py ${1:-1000000} ${2:-50000} ${3:-1023} ${4:-5} 2>&1 | tee "$O/ld_op.txt" || exit 1
  cp -f "$O/ld_op.txt" "$R/profiles/r14_ld_op.txt" ;;
assoc)
  # whole-call time of the scan per shape and data set beside the bare 'T' product of the same run, alternating calls; the text is what profiles/r15_assoc.txt holds
  timeout -k 10 900 python3 tools/perf_assoc.py ${1:-1000000} ${2:-50000} ${3:-5} 2>&1 | tee "$O/assoc.txt" || exit 1
  cp -f "$O/assoc.txt" "$R/profiles/r15_assoc.txt" ;;
assoc-kernels)
  # per-kernel times of the second call of each data set and shape; the text is what profiles/r15_assoc_kernels.txt holds
  D="$O/assoc_trace"; rm -rf "$D"; mkdir -p "$D"
  ( cd /tmp && timeout -k 10 600 rocprofv3 --kernel-trace --output-format csv -d "$D" -- python3 "$R/tools/perf_assoc.py" ${1:-1000000} ${2:-50000} trace > "$O/assoc_trace_run.log" 2>&1 ) || { tail -5 "$O/assoc_trace_run.log"; exit 1; }
  f=$(find "$D" -name '*kernel_trace.csv' | head -1) && python3 tools/perf_assoc.py summarize "$f" 2>&1 | tee "$O/assoc_kernels.txt" || exit 1
  rm -rf "$D"; cp -f "$O/assoc_kernels.txt" "$R/profiles/r15_assoc_kernels.txt" ;;
assoc-score)
  # whole-call time of the score test per shape and data set beside the linear entry and the bare 'T' products of the same run; the text is what profiles/r16_assoc_score.txt holds
  timeout -k 10 900 python3 tools/perf_assoc.py score ${1:-1000000} ${2:-50000} ${3:-5} 2>&1 | tee "$O/assoc_score.txt" || exit 1
  cp -f "$O/assoc_score.txt" "$R/profiles/r16_assoc_score.txt" ;;
assoc-score-kernels)
  # per-kernel times of the second call of each data set and shape; the text is what profiles/r16_assoc_score_kernels.txt holds
  D="$O/assoc_score_trace"; rm -rf "$D"; mkdir -p "$D"
  ( cd /tmp && timeout -k 10 600 rocprofv3 --kernel-trace --output-format csv -d "$D" -- python3 "$R/tools/perf_assoc.py" score ${1:-1000000} ${2:-50000} trace > "$O/assoc_score_trace_run.log" 2>&1 ) || { tail -5 "$O/assoc_score_trace_run.log"; exit 1; }
  f=$(find "$D" -name '*kernel_trace.csv' | head -1) && python3 tools/perf_assoc.py summarize-score "$f" 2>&1 | tee "$O/assoc_score_kernels.txt" || exit 1
  rm -rf "$D"; cp -f "$O/assoc_score_kernels.txt" "$R/profiles/r16_assoc_score_kernels.txt" ;;
assoc-spa)
  # whole-call time of the entry beside mxa_assoc_score of the same run, alternating calls; the text is what profiles/r17_assoc_spa.txt holds
  timeout -k 10 900 python3 tools/perf_assoc_spa.py ${1:-50000} ${2:-1000000} ${3:-5} 2>&1 | tee "$O/assoc_spa.txt" || exit 1
  cp -f "$O/assoc_spa.txt" "$R/profiles/r17_assoc_spa.txt" ;;
assoc-spa-kernels)
  # per-kernel times of the second call; the text is what profiles/r17_assoc_spa_kernels.txt holds
  D="$O/assoc_spa_trace"; rm -rf "$D"; mkdir -p "$D"
  ( cd /tmp && timeout -k 10 600 rocprofv3 --kernel-trace --output-format csv -d "$D" -- python3 "$R/tools/perf_assoc_spa.py" ${1:-50000} ${2:-1000000} trace > "$O/assoc_spa_trace_run.log" 2>&1 ) || { tail -5 "$O/assoc_spa_trace_run.log"; exit 1; }
  f=$(find "$D" -name '*kernel_trace.csv' | head -1) && python3 tools/perf_assoc_spa.py summarize "$f" 2>&1 | tee "$O/assoc_spa_kernels.txt" || exit 1
  rm -rf "$D"; cp -f "$O/assoc_spa_kernels.txt" "$R/profiles/r17_assoc_spa_kernels.txt" ;;
assoc-firth)
  # whole-call times of the entry beside mxa_assoc_score and mxa_assoc_score_spa of the same run, alternating calls; the text is what profiles/r18_assoc_firth.txt holds
  timeout -k 10 900 python3 tools/perf_assoc_firth.py ${1:-50000} ${2:-1000000} ${3:-7} 2>&1 | tee "$O/assoc_firth.txt" || exit 1
  cp -f "$O/assoc_firth.txt" "$R/profiles/r18_assoc_firth.txt" ;;
assoc-firth-kernels)
  # per-kernel times of each entry's second call; the text is what profiles/r18_assoc_firth_kernels.txt holds
  D="$O/assoc_firth_trace"; rm -rf "$D"; mkdir -p "$D"
  ( cd /tmp && timeout -k 10 800 rocprofv3 --kernel-trace --output-format csv -d "$D" -- python3 "$R/tools/perf_assoc_firth.py" ${1:-50000} ${2:-1000000} trace > "$O/assoc_firth_trace_run.log" 2>&1 ) || { tail -5 "$O/assoc_firth_trace_run.log"; exit 1; }
  f=$(find "$D" -name '*kernel_trace.csv' | head -1) && python3 tools/perf_assoc_firth.py summarize "$f" "$O/assoc_firth_trace_run.log" 2>&1 | tee "$O/assoc_firth_kernels.txt" || exit 1
  rm -rf "$D"; cp -f "$O/assoc_firth_kernels.txt" "$R/profiles/r18_assoc_firth_kernels.txt" ;;
assoc-set)
  # whole-call times of the entry beside mxa_assoc_score of the same run, alternating calls, and the torch route; the text is what profiles/r19_assoc_set.txt holds
  timeout -k 10 900 python3 tools/perf_assoc_set.py ${1:-50000} ${2:-1000000} ${3:-7} 2>&1 | tee "$O/assoc_set.txt" || exit 1
  cp -f "$O/assoc_set.txt" "$R/profiles/r19_assoc_set.txt" ;;
assoc-set-kernels)
  # per-kernel times of the second call at each set size; the text is what profiles/r19_assoc_set_kernels.txt holds
  D="$O/assoc_set_trace"; rm -rf "$D"; mkdir -p "$D"
  ( cd /tmp && timeout -k 10 800 rocprofv3 --kernel-trace --output-format csv -d "$D" -- python3 "$R/tools/perf_assoc_set.py" ${1:-50000} ${2:-1000000} trace > "$O/assoc_set_trace_run.log" 2>&1 ) || { tail -5 "$O/assoc_set_trace_run.log"; exit 1; }
  f=$(find "$D" -name '*kernel_trace.csv' | head -1) && python3 tools/perf_assoc_set.py summarize "$f" 2>&1 | tee "$O/assoc_set_kernels.txt" || exit 1
  rm -rf "$D"; cp -f "$O/assoc_set_kernels.txt" "$R/profiles/r19_assoc_set_kernels.txt" ;;
assoc-mixed)
  # whole-call time of one assoc_mixed call with the split gram / scan / everything else from HIP events, then the kernel classes of a traced run of its own; the text is what profiles/r20_assoc_mixed.txt holds
  timeout -k 10 900 python3 tools/perf_assoc_mixed.py ${1:-50000} ${2:-1000000} ${3:-5} 2>&1 | tee "$O/assoc_mixed.txt" || exit 1
  D="$O/assoc_mixed_trace"; rm -rf "$D"; mkdir -p "$D"
  ( cd /tmp && timeout -k 10 900 rocprofv3 --kernel-trace --output-format csv -d "$D" -- python3 "$R/tools/perf_assoc_mixed.py" ${1:-50000} ${2:-1000000} ${3:-5} trace > "$O/assoc_mixed_trace_run.log" 2>&1 ) || { tail -5 "$O/assoc_mixed_trace_run.log"; exit 1; }
  f=$(find "$D" -name '*kernel_trace.csv' | head -1) && python3 tools/perf_assoc_mixed.py summarize "$f" 2>&1 | tee -a "$O/assoc_mixed.txt" || exit 1
  rm -rf "$D"; cp -f "$O/assoc_mixed.txt" "$R/profiles/r20_assoc_mixed.txt" ;;
gemm)
  timeout -k 10 600 python3 tools/perf_gemm.py "$@" 2>&1 | tee -a "$O/gemm.txt" ;;
rehearse)
  timeout -k 10 500 python bench.py --full --gpus 8 --steps 5 --warmup 1 > "$O/bench_inprocess_8_virtual_shards.json" 2> "$O/inprocess8.err" || { tail -5 "$O/inprocess8.err"; exit 1; }
  cp -f bench_detail.json "$O/bench_detail_inprocess_8_virtual_shards.json"
  for n in 2 4; do
    MXA_BENCH_SINGLE_DEVICE=1 MXA_BENCH_BACKEND=gloo timeout -k 10 500 python -m torch.distributed.run --nnodes=1 --nproc-per-node $n --master-addr 127.0.0.1 --master-port 2957$n \
      bench.py --full --gpus $n --steps 5 --warmup 1 > "$O/launcher_${n}ranks.log" 2>&1 || { tail -5 "$O/launcher_${n}ranks.log"; exit 1; }
    grep '^{' "$O/launcher_${n}ranks.log" > "$O/bench_launcher_${n}_ranks_one_gpu_gloo.json"
  done
  for f in "$O"/bench_inprocess_8_virtual_shards.json "$O"/bench_launcher_*_ranks_one_gpu_gloo.json; do echo "== $f"; cat "$f"; done ;;
soak)
  timeout -k 10 500 python3 tools/soak.py 2>&1 | tail -5 | tee "$O/soak.txt" &&
  timeout -k 10 400 python3 tools/fuzz_shapes.py 2>&1 | tail -3 | tee -a "$O/soak.txt" &&
  timeout -k 10 400 python3 tools/fuzz_crossprod.py 2>&1 | tail -3 | tee -a "$O/soak.txt" ;;
*)
  sed -n 2,20p "$0"; exit 2 ;;
esac
