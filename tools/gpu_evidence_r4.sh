#!/bin/bash
# Round-4 evidence: default bench line, kernel traces of the same command (co-visitation + kNN + config 5),
# PMC FETCH / WRITE per phase (profiles/r4_pmc_traffic.json via tools/pmc_phases.py) and per-kernel SQ mix
set -o pipefail
O=gpurun_out/${1:-ev_r4}; mkdir -p $O
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
B="bench.py --full --steps 1 --warmup 0 --knn-steps 1 --cand-steps 0 --no-cpu --no-a6 --no-ingest"
timeout -s KILL 180 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $O/f -o run -- python3 $B > $O/f.log 2>&1 || { tail -20 $O/f.log; exit 1; }
timeout -s KILL 180 rocprofv3 --pmc WRITE_SIZE --output-format csv -d $O/w -o run -- python3 $B > $O/w.log 2>&1 || { tail -20 $O/w.log; exit 1; }
python3 tools/pmc_phases.py $O/f/run_counter_collection.csv $O/w/run_counter_collection.csv > $O/r4_pmc_traffic.json || exit 1
timeout -s KILL 180 rocprofv3 --kernel-trace --stats --output-format csv -d $O/k -o run -- python3 $B > $O/k.log 2>&1 || { tail -20 $O/k.log; exit 1; }
timeout -s KILL 180 rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_LDS SQ_INSTS_SALU SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_INSTS_VMEM_WR SQ_INSTS_VMEM_RD --output-format csv -d $O/a -o run -- python3 $B > $O/a.log 2>&1 || { tail -20 $O/a.log; exit 1; }
python3 tools/kpmc_table.py $O 40 > $O/pmc_per_kernel.txt 2>&1; head -30 $O/pmc_per_kernel.txt
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $O/full -o run -- python3 -u bench.py --full --no-cpu --steps 3 --warmup 1 > $O/full.log 2>&1 || { tail -20 $O/full.log; exit 1; }
python3 tools/kstats.py $O/full/run_kernel_stats.csv > $O/full_summary.txt; head -25 $O/full_summary.txt
timeout -k 10 600 python3 -u bench.py --full > $O/bench.log 2>&1 || { tail -30 $O/bench.log; exit 1; }
grep '^{' $O/bench.log | tail -1 > $O/bench.json
python3 -c "import json,sys; d=json.load(open(sys.argv[1])); print(d['ms_per_step'], d['phases_ms'], d['roofline']['frac'], d['knn']['phases_ms'], d['candidates']['ms_per_step'], d['a6']['total_ms'])" $O/bench.json
