#!/bin/bash
# usage (GPU box): bash scripts/gpu_r4.sh <run> [args]   -- the round-4 measurement runs, one function per run.
# (formerly scripts/gpu_r4_<run>.sh; profiles/r04_*.md cite them under those names)
set -u

run_b() {
# Round 4, second GPU session: plan + pool forward (parity, timing, counters), BN finish kernel, graph-replay diag.
R=$PWD
OUT=$R/gpurun_out/r4_b; mkdir -p $OUT
export TMPDIR=/tmp
timeout 900 python -m pytest tests/test_gpu_roi_align.py tests/test_gpu_frozen_bn.py -x -q -k "sliced or golden or cfg0 or full_size or channels_last or riroi_vector or frozen or bn or bias" > $OUT/pytest.log 2>&1
echo "pytest rc=$?"; tail -4 $OUT/pytest.log
trace() {  # $1 = tag, rest = env
  tag=$1; shift
  (cd /tmp && env "$@" timeout 300 rocprofv3 --kernel-trace --output-format csv -d $OUT/t_$tag -o t -- python $R/bench.py --workload roi_align_rotated --no-cpu-baseline --no-secondary --steps 50 > $OUT/t_$tag.log 2>&1)
  python - <<PY
import csv,glob,collections,re
f=glob.glob("$OUT/t_$tag/**/*kernel_trace.csv",recursive=True)
d=collections.defaultdict(list)
for r in csv.DictReader(open(f[0])):
    m=re.search(r"(roi_\w+_kernel)", r["Kernel_Name"]); k=m.group(1) if m else r["Kernel_Name"][:30]
    d[k].append((int(r["End_Timestamp"])-int(r["Start_Timestamp"]))/1e3)
print("[$tag]", "; ".join("%s %.1f"%(k,sum(v[5:])/len(v[5:])) for k,v in d.items() if len(v)>5))
PY
}
trace default A=1
trace pred JDET_ROI_SLICED_PRED=1
trace b4 JDET_ROI_SLICED_BATCH=4
trace b4pred JDET_ROI_SLICED_BATCH=4 JDET_ROI_SLICED_PRED=1
trace b16 JDET_ROI_SLICED_BATCH=16
trace legacy JDET_ROI_FWD_LEGACY=1
pmc() {  # $1 = tag, $2 = counters, rest = env
  tag=$1; c=$2; shift; shift
  (cd /tmp && env "$@" timeout 300 rocprofv3 --pmc $c --output-format csv -d $OUT/p_$tag -o t -- python $R/bench.py --workload roi_align_rotated --no-cpu-baseline --no-secondary --steps 10 --warmup 3 > $OUT/p_$tag.log 2>&1)
  python - <<PY
import csv,glob,collections,re
for f in sorted(glob.glob("$OUT/p_$tag/**/*counter_collection.csv",recursive=True)):
    d=collections.defaultdict(lambda: collections.defaultdict(list))
    for r in csv.DictReader(open(f)):
        m=re.search(r"(roi_\w+_kernel)", r["Kernel_Name"])
        if m: d[m.group(1)][r["Counter_Name"]].append(float(r["Counter_Value"]))
    for k,v in d.items(): print("[$tag]", k, {c: round(sum(x)/len(x)) for c,x in v.items()})
PY
}
pmc ea "TCC_EA0_RDREQ_sum TCC_READ_sum" A=1
pmc hit "TCC_HIT_sum TCC_MISS_sum" A=1
pmc fetch "FETCH_SIZE" A=1
pmc write "WRITE_SIZE" A=1
pmc tcp "TCP_TCC_READ_REQ_sum TCP_TOTAL_CACHE_ACCESSES_sum" A=1
pmc sq "SQ_WAVES SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_INSTS_VALU SQ_INSTS_VMEM_RD" A=1
timeout 120 python bench.py --workload roi_align_rotated --no-cpu-baseline --no-secondary 2>/dev/null | tail -1 | cut -c1-400
# two ranks on one device, graph mode, probes at every hand-over (scripts/ddp_graph_diag.py)
timeout 900 python scripts/ddp_graph_diag.py orcnn 9 4 > $OUT/ddp_diag.log 2>&1
grep -E "^== run|RESULT|DISAGREE|GARBAGE|Error|error" $OUT/ddp_diag.log | cut -c1-400 | head -40
}

run_d() {
# Round 4, forward experiments: workgroup size of the pool kernel, slice-planar map layout (L2 channel spread test)
R=$PWD
OUT=$R/gpurun_out/r4_d; mkdir -p $OUT
export TMPDIR=/tmp
trace() {  # $1 = tag, rest = env
  tag=$1; shift
  (cd /tmp && env JDET_BENCH_CHECKSUM=1 "$@" timeout 300 rocprofv3 --kernel-trace --output-format csv -d $OUT/t_$tag -o t -- python $R/bench.py --workload roi_align_rotated --no-cpu-baseline --no-secondary --steps 50 > $OUT/t_$tag.log 2>&1)
  python - <<PY
import csv,glob,collections,re
f=glob.glob("$OUT/t_$tag/**/*kernel_trace.csv",recursive=True)
d=collections.defaultdict(list)
for r in csv.DictReader(open(f[0])):
    m=re.search(r"(roi_\w+_kernel)", r["Kernel_Name"]); k=m.group(1) if m else r["Kernel_Name"][:30]
    d[k].append((int(r["End_Timestamp"])-int(r["Start_Timestamp"]))/1e3)
cs=[l.strip() for l in open("$OUT/t_$tag.log") if l.startswith("checksum")]
print("[$tag]", "; ".join("%s %.1f"%(k,sum(v[5:])/len(v[5:])) for k,v in d.items() if len(v)>5), "|", cs[-1] if cs else "")
PY
}
trace b4pred JDET_ROI_FWD_SLICED=1 JDET_ROI_SLICED_BATCH=4 JDET_ROI_SLICED_PRED=1
trace b4pred_w8 JDET_ROI_FWD_SLICED=1 JDET_ROI_SLICED_BATCH=4 JDET_ROI_SLICED_PRED=1 JDET_ROI_SLICED_WAVES=8
trace b4pred_w16 JDET_ROI_FWD_SLICED=1 JDET_ROI_SLICED_BATCH=4 JDET_ROI_SLICED_PRED=1 JDET_ROI_SLICED_WAVES=16
trace b4pred_w1 JDET_ROI_FWD_SLICED=1 JDET_ROI_SLICED_BATCH=4 JDET_ROI_SLICED_PRED=1 JDET_ROI_SLICED_WAVES=1
trace w16 JDET_ROI_FWD_SLICED=1 JDET_ROI_SLICED_WAVES=16
trace planar JDET_ROI_FWD_SLICED=1 JDET_ROI_SLICED_PLANAR=1 JDET_ROI_SLICED_BATCH=4 JDET_ROI_SLICED_PRED=1
trace planar_w16 JDET_ROI_FWD_SLICED=1 JDET_ROI_SLICED_PLANAR=1 JDET_ROI_SLICED_BATCH=4 JDET_ROI_SLICED_PRED=1 JDET_ROI_SLICED_WAVES=16
trace legacy A=1
pmc() {  # $1 = tag, $2 = counters, rest = env
  tag=$1; c=$2; shift; shift
  (cd /tmp && env "$@" timeout 300 rocprofv3 --pmc $c --output-format csv -d $OUT/p_$tag -o t -- python $R/bench.py --workload roi_align_rotated --no-cpu-baseline --no-secondary --steps 10 --warmup 3 > $OUT/p_$tag.log 2>&1)
  python - <<PY
import csv,glob,collections,re
for f in sorted(glob.glob("$OUT/p_$tag/**/*counter_collection.csv",recursive=True)):
    d=collections.defaultdict(lambda: collections.defaultdict(list))
    for r in csv.DictReader(open(f)):
        m=re.search(r"(roi_pool\w+_kernel)", r["Kernel_Name"])
        if m: d[m.group(1)][r["Counter_Name"]].append(float(r["Counter_Value"]))
    for k,v in d.items(): print("[$tag]", k, {c: round(sum(x)/len(x)) for c,x in v.items()})
PY
}
P="JDET_ROI_FWD_SLICED=1 JDET_ROI_SLICED_PLANAR=1 JDET_ROI_SLICED_BATCH=4 JDET_ROI_SLICED_PRED=1"
pmc planar_ea "TCC_EA0_RDREQ_sum TCC_READ_sum" $P
pmc planar_hit "TCC_HIT_sum TCC_MISS_sum" $P
pmc planar_sq "SQ_WAVES SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_INSTS_VALU SQ_INSTS_VMEM_RD" $P
pmc planar_tcp "TCP_TCC_READ_REQ_sum TCP_TOTAL_CACHE_ACCESSES_sum" $P
rocprofv3 -L 2>/dev/null | grep -o "TCP_[A-Z_0-9]*\|TCC_[A-Z_0-9]*STALL[A-Z_0-9]*\|TA_[A-Z_0-9]*" | sort -u | tr '\n' ' ' | cut -c1-3000
}

run_e() {
# Round 4: backward with 4x4 patches (parity + A/B against the 2x2 path), RiRoIAlign forward after the mix rewrite
R=$PWD
OUT=$R/gpurun_out/r4_e; mkdir -p $OUT
export TMPDIR=/tmp
timeout 1200 python -m pytest tests/test_gpu_roi_align.py tests/test_gpu_closed_form.py -x -q > $OUT/pytest.log 2>&1
echo "pytest rc=$?"; tail -4 $OUT/pytest.log
timeout 600 python -m pytest tests/test_gpu_reference_kernels.py -x -q -k "roi" > $OUT/pytest_ref.log 2>&1
echo "pytest ref rc=$?"; tail -3 $OUT/pytest_ref.log
trace() {  # $1 = tag, $2 = workload, rest = env
  tag=$1; wl=$2; shift; shift
  (cd /tmp && env JDET_BENCH_CHECKSUM=1 "$@" timeout 300 rocprofv3 --kernel-trace --output-format csv -d $OUT/t_$tag -o t -- python $R/bench.py --workload $wl --no-cpu-baseline --no-secondary --steps 50 > $OUT/t_$tag.log 2>&1)
  python - <<PY
import csv,glob,collections,re
f=glob.glob("$OUT/t_$tag/**/*kernel_trace.csv",recursive=True)
d=collections.defaultdict(list)
for r in csv.DictReader(open(f[0])):
    m=re.search(r"((roi|csr|bwd|riroi)_\w+_kernel)", r["Kernel_Name"]); k=m.group(1) if m else r["Kernel_Name"][:30]
    d[k].append((int(r["End_Timestamp"])-int(r["Start_Timestamp"]))/1e3)
cs=[l.strip() for l in open("$OUT/t_$tag.log") if l.startswith("checksum")]
tot=sum(sum(v[5:])/len(v[5:]) for k,v in d.items() if len(v)>5)
print("[$tag] total %.1f :"%tot, "; ".join("%s %.1f"%(k,sum(v[5:])/len(v[5:])) for k,v in d.items() if len(v)>5), "|", cs[-1] if cs else "")
PY
}
trace bwd4 roi_align_rotated_bwd A=1
trace bwd2 roi_align_rotated_bwd JDET_ROI_BWD_PATCH=2
trace riroi riroi_align A=1
trace fwd roi_align_rotated A=1
for wl in roi_align_rotated_bwd riroi_align roi_align_rotated; do timeout 120 python bench.py --workload $wl --no-cpu-baseline --no-secondary 2>/dev/null | tail -1 | python -c 'import sys,json; d=json.loads(sys.stdin.readline()); print(d["config"]["workload"], round(d["ms_per_step"]*1000,1),"us/step frac", round(d["roofline"]["frac"],3))'; done
}

run_f() {
# Round 4: backward producer rewrite (independent atomics, scan folded in), RiRoIAlign static mix, full-size pins against
# the reference's kernels, reference-kernel timings, S2ANet step after the BN finish change, two-rank graph test x3
R=$PWD
OUT=$R/gpurun_out/r4_f; mkdir -p $OUT
export TMPDIR=/tmp
timeout 1500 python -m pytest tests/test_gpu_roi_align.py tests/test_gpu_closed_form.py tests/test_gpu_reference_kernels.py -q > $OUT/pytest.log 2>&1
echo "pytest rc=$?"; tail -4 $OUT/pytest.log
trace() {  # $1 = tag, $2 = workload, rest = env
  tag=$1; wl=$2; shift; shift
  (cd /tmp && env JDET_BENCH_CHECKSUM=1 "$@" timeout 300 rocprofv3 --kernel-trace --output-format csv -d $OUT/t_$tag -o t -- python $R/bench.py --workload $wl --no-cpu-baseline --no-secondary --steps 50 > $OUT/t_$tag.log 2>&1)
  python - <<PY
import csv,glob,collections,re
f=glob.glob("$OUT/t_$tag/**/*kernel_trace.csv",recursive=True)
d=collections.defaultdict(list)
for r in csv.DictReader(open(f[0])):
    m=re.search(r"((roi|csr|bwd|riroi)_\w+_kernel)", r["Kernel_Name"]); k=m.group(1) if m else r["Kernel_Name"][:30]
    d[k].append((int(r["End_Timestamp"])-int(r["Start_Timestamp"]))/1e3)
cs=[l.strip() for l in open("$OUT/t_$tag.log") if l.startswith("checksum")]
tot=sum(sum(v[5:])/len(v[5:]) for k,v in d.items() if len(v)>5)
print("[$tag] total %.1f :"%tot, "; ".join("%s %.1f"%(k,sum(v[5:])/len(v[5:])) for k,v in d.items() if len(v)>5), "|", cs[-1] if cs else "")
PY
}
trace bwd roi_align_rotated_bwd A=1
trace riroi riroi_align A=1
for wl in roi_align_rotated_bwd riroi_align roi_align_rotated; do timeout 120 python bench.py --workload $wl --no-cpu-baseline --no-secondary 2>/dev/null | tail -1 | python -c 'import sys,json; d=json.loads(sys.stdin.readline()); print(d["config"]["workload"], round(d["ms_per_step"]*1000,1),"us/step frac", round(d["roofline"]["frac"],3))'; done
# the reference's own RoIAlign kernels on this GPU (kernel durations from the trace)
(cd /tmp && timeout 300 rocprofv3 --kernel-trace --output-format csv -d $OUT/t_refk -o t -- python $R/scripts/refk_diag.py --time > $OUT/refk_time.log 2>&1)
tail -3 $OUT/refk_time.log
python - <<PY
import csv,glob,collections
f=glob.glob("$OUT/t_refk/**/*kernel_trace.csv",recursive=True)
d=collections.defaultdict(list)
for r in csv.DictReader(open(f[0])):
    d[r["Kernel_Name"][:90]].append((int(r["End_Timestamp"])-int(r["Start_Timestamp"]))/1e3)
for k,v in sorted(d.items(), key=lambda kv:-sum(kv[1])):
    if len(v)>=10: print("  %-90s n=%d avg %.1f us"%(k,len(v),sum(v[2:])/len(v[2:])))
PY
timeout 600 python bench.py --steps 20 --warmup 5 --no-cpu-baseline --no-secondary 2>/dev/null | tail -1 | python -c 'import sys,json; d=json.loads(sys.stdin.readline()); print("s2anet", d["value"], "img/s", d["ms_per_step"], "ms; roofline", d["roofline"]["frac"], d["roofline"]["kernel_ms"])'
for i in 1 2; do timeout 600 python -m pytest tests/test_gpu_ddp_detectors.py -q -k "graph" --runxfail > $OUT/ddp_$i.log 2>&1; tail -1 $OUT/ddp_$i.log; grep -E "^FAILED|AssertionError|replicas diverged" $OUT/ddp_$i.log | cut -c1-600 | head -6; done
}

run_final() {
# round 4 evidence run: smoke(), the full GPU suite, the default bench line, the same command under rocprofv3
# (steady-state step breakdown + roofline-kernel rows), traffic counters of the roofline kernel (one --pmc set per pass),
# kernel stats of backward / RiRoIAlign / IoU / NMS, MFMA counters of the whole S2ANet step, the other model workloads.
# Output: gpurun_out/r4_final/ (what is judged is copied into profiles/r04_*).
R=$PWD
OUT=$R/gpurun_out/r4_final; mkdir -p $OUT
export TMPDIR=/tmp
timeout 300 python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -1
timeout 2400 python -m pytest tests -m gpu -q > $OUT/pytest_gpu.log 2>&1; tail -2 $OUT/pytest_gpu.log
timeout 900 python bench.py --full > $OUT/bench_default.json 2> $OUT/bench_default.err; tail -1 $OUT/bench_default.json | cut -c1-900
(cd /tmp && timeout 900 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/trace_default -o t -- python $R/bench.py --steps 8 --warmup 4 --full --no-live-traffic --no-cpu-baseline --no-secondary > $OUT/trace_default.log 2>&1)
f=$(find $OUT/trace_default -name '*kernel_trace.csv' | head -1)
python scripts/steady_state.py $f assign_anchor_kernel 4 5 120 > $OUT/steady_state_s2anet.txt 2>&1
head -3 $OUT/steady_state_s2anet.txt | cut -c1-160
k=$(find $OUT/trace_default -name '*kernel_stats.csv' | head -1)
head -1 $k > $OUT/roofline_kernel_stats.csv
grep "roi_align_fwd_merged_kernel\|roi_order_kernel\|conv3x3_igemm_kernel\|sums_finish_kernel\|bias_act_bwd_kernel" $k >> $OUT/roofline_kernel_stats.csv
cut -c1-240 $OUT/roofline_kernel_stats.csv
rm -rf $OUT/trace_default
# traffic of the roofline kernel (default path), one counter set per pass
for c in "FETCH_SIZE" "WRITE_SIZE" "TCC_READ_sum TCC_EA0_RDREQ_sum TCC_HIT_sum TCC_MISS_sum" "TCP_TOTAL_CACHE_ACCESSES_sum TCP_TCC_READ_REQ_sum SQ_INSTS_VMEM_RD SQ_INSTS_VALU SQ_WAVE_CYCLES SQ_WAIT_INST_ANY"; do
  n=$(echo $c | tr ' ' '_' | cut -c1-30)
  (cd /tmp && timeout 300 rocprofv3 --pmc $c --output-format csv -d $OUT/pmc_fwd_$n -o p -- python $R/bench.py --workload roi_align_rotated --no-cpu-baseline --no-secondary --steps 10 --warmup 3 > $OUT/pmc_fwd_$n.log 2>&1)
done
python - <<PY > $OUT/roi_align_fwd_counters.txt
import csv, glob, collections
agg = collections.defaultdict(lambda: collections.defaultdict(list))
for f in glob.glob("$OUT/pmc_fwd_*/**/*counter_collection.csv", recursive=True):
    for row in csv.DictReader(open(f)):
        agg[row["Kernel_Name"][:70]][row["Counter_Name"]].append(float(row["Counter_Value"]))
for k, cs in agg.items():
    if "roi_" in k:
        for c, v in sorted(cs.items()):
            print("%-70s %-32s mean %.6g over %d dispatches" % (k, c, sum(v) / len(v), len(v)))
PY
cut -c40-200 $OUT/roi_align_fwd_counters.txt
rm -rf $OUT/pmc_fwd_*/
for wl in roi_align_rotated roi_align_rotated_bwd riroi_align box_iou_rotated nms_rotated; do
  (cd /tmp && timeout 400 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/trace_$wl -o t -- python $R/bench.py --workload $wl --no-cpu-baseline --no-secondary > $OUT/trace_$wl.log 2>&1)
  k=$(find $OUT/trace_$wl -name '*kernel_stats.csv' | head -1)
  [ -n "$k" ] && head -12 $k | cut -c1-220 > $OUT/kernel_stats_$wl.csv
  grep -o '"ms_per_step": [0-9.]*' $OUT/trace_$wl.log | head -1
  rm -rf $OUT/trace_$wl
  echo "== $wl"; cut -c1-150 $OUT/kernel_stats_$wl.csv | head -7
done
# MFMA counters over the S2ANet step (two passes)
for c in "SQ_INSTS_VALU_MFMA_MOPS_F32 SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES" "SQ_INSTS_MFMA SQ_INSTS_VALU GRBM_GUI_ACTIVE"; do
  n=$(echo $c | tr ' ' '_' | cut -c1-40)
  (cd /tmp && timeout 900 rocprofv3 --pmc $c -f csv -d $OUT/mfma_$n -o p -- python $R/bench.py --steps 3 --warmup 3 --no-cpu-baseline --no-secondary > $OUT/mfma_$n.log 2>&1 || echo "pmc $c failed")
done
python - <<PY
import csv, glob, collections
tot = collections.defaultdict(lambda: collections.defaultdict(float))
cnt = collections.defaultdict(lambda: collections.defaultdict(int))
for f in glob.glob("$OUT/mfma_*/**/*counter_collection.csv", recursive=True):
    for row in csv.DictReader(open(f)):
        k = row["Kernel_Name"][:90]
        tot[k][row["Counter_Name"]] += float(row["Counter_Value"])
        cnt[k][row["Counter_Name"]] += 1
rows = sorted(tot.items(), key=lambda kv: -kv[1].get("SQ_VALU_MFMA_BUSY_CYCLES", 0))[:25]
busy_all = act_all = 0.0
with open("$OUT/s2anet_mfma_utilisation.txt", "w") as o:
    o.write("# MFMA busy = SQ_VALU_MFMA_BUSY_CYCLES / (GRBM_GUI_ACTIVE / 8 XCDs x 1024 SIMDs); GFLOP = SQ_INSTS_VALU_MFMA_MOPS_F32 x 512 / 1e9;\n# S2ANet-R50-FPN train step 2 x 1024^2 (bench.py --steps 3 --warmup 3), two --pmc passes, the 25 kernels with most MFMA-busy cycles\n")
    o.write("%-90s %6s %9s %11s\n" % ("kernel", "disp", "MFMA busy", "GFLOP/disp"))
    for k, v in rows:
        d = max(cnt[k].get("SQ_VALU_MFMA_BUSY_CYCLES", 1), 1)
        gui = v.get("GRBM_GUI_ACTIVE", 0.0) * d / max(cnt[k].get("GRBM_GUI_ACTIVE", 1), 1)
        busy = v.get("SQ_VALU_MFMA_BUSY_CYCLES", 0.0) / (gui / 8 * 1024) if gui else 0.0
        busy_all += v.get("SQ_VALU_MFMA_BUSY_CYCLES", 0.0); act_all += gui / 8 * 1024
        o.write("%-90s %6d %8.1f%% %11.2f\n" % (k, d, 100 * busy, v.get("SQ_INSTS_VALU_MFMA_MOPS_F32", 0.0) * 512 / 1e9 / d))
    o.write("cycle-weighted MFMA busy over these 25 kernels: %.1f%%\n" % (100 * busy_all / act_all if act_all else 0))
print(open("$OUT/s2anet_mfma_utilisation.txt").read()[:3500])
PY
rm -rf $OUT/mfma_SQ*
for wl in retinanet_infer orcnn_train roitrans_r50_train roitrans_train; do
  timeout 600 python bench.py --workload $wl --no-cpu-baseline --no-secondary > $OUT/bench_$wl.json 2> $OUT/bench_$wl.err
  python -c "
import json,sys
l=json.loads(open('$OUT/bench_$wl.json').read().strip().splitlines()[-1]); print('$wl', l['ms_per_step'], 'ms/step', l['value'], l['unit'], l['config'].get('global_batch'))" 2>/dev/null || echo "$wl failed"
done
ls $OUT
}

run_fwd() {
# Round 4, forward: parity of the channel-sliced kernel, then kernel-trace averages and traffic counters of the
# product path under its tuning knobs and of the legacy (RoI-stationary) kernels.  -> gpurun_out/r4_fwd/
R=$PWD
OUT=$R/gpurun_out/r4_fwd; mkdir -p $OUT
export TMPDIR=/tmp
timeout 900 python -m pytest tests/test_gpu_roi_align.py -x -q -k "sliced or golden or cfg0 or full_size or channels_last or riroi_vector" > $OUT/pytest.log 2>&1
echo "pytest rc=$?"; tail -5 $OUT/pytest.log
trace() {  # $1 = tag, rest = env
  tag=$1; shift
  (cd /tmp && env "$@" timeout 300 rocprofv3 --kernel-trace --output-format csv -d $OUT/t_$tag -o t -- python $R/bench.py --workload roi_align_rotated --no-cpu-baseline --no-secondary --steps 50 > $OUT/t_$tag.log 2>&1)
  python - <<PY
import csv,glob,collections
f=glob.glob("$OUT/t_$tag/**/*kernel_trace.csv",recursive=True)
d=collections.defaultdict(list)
for r in csv.DictReader(open(f[0])): d[r["Kernel_Name"].split("::")[-1][:40]].append((int(r["End_Timestamp"])-int(r["Start_Timestamp"]))/1e3)
print("[$tag]", "; ".join("%s %.1f"%(k,sum(v[5:])/len(v[5:])) for k,v in d.items() if len(v)>5), "|", open("$OUT/t_$tag.log").read().strip().split("\n")[-1][:160])
PY
}
trace default A=1
trace b4 JDET_ROI_SLICED_BATCH=4
trace b16 JDET_ROI_SLICED_BATCH=16
trace plain JDET_ROI_SLICED_STORE=1
trace sc1 JDET_ROI_SLICED_STORE=2
trace b16plain JDET_ROI_SLICED_BATCH=16 JDET_ROI_SLICED_STORE=1
trace legacy JDET_ROI_FWD_LEGACY=1
pmc() {  # $1 = tag, $2 = counters, rest = env
  tag=$1; c=$2; shift; shift
  (cd /tmp && env "$@" timeout 300 rocprofv3 --pmc $c --output-format csv -d $OUT/p_$tag -o t -- python $R/bench.py --workload roi_align_rotated --no-cpu-baseline --no-secondary --steps 10 --warmup 3 > $OUT/p_$tag.log 2>&1)
  python - <<PY
import csv,glob,collections
for f in sorted(glob.glob("$OUT/p_$tag/**/*counter_collection.csv",recursive=True)):
    d=collections.defaultdict(lambda: collections.defaultdict(list))
    for r in csv.DictReader(open(f)):
        d[r["Kernel_Name"].split("::")[-1][:28]][r["Counter_Name"]].append(float(r["Counter_Value"]))
    for k,v in d.items():
        if "roi_" in k: print("[$tag]", k, {c: round(sum(x)/len(x)) for c,x in v.items()})
PY
}
for v in default legacy; do
  e="A=1"; [ $v = legacy ] && e="JDET_ROI_FWD_LEGACY=1"
  pmc ${v}_ea "TCC_EA0_RDREQ_sum TCC_READ_sum" $e
  pmc ${v}_hit "TCC_HIT_sum TCC_MISS_sum" $e
  pmc ${v}_fetch "FETCH_SIZE" $e
  pmc ${v}_write "WRITE_SIZE" $e
  pmc ${v}_tcp "TCP_TCC_READ_REQ_sum TCP_TOTAL_CACHE_ACCESSES_sum" $e
  pmc ${v}_sq "SQ_WAVES SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_INSTS_VALU SQ_INSTS_VMEM_RD" $e
done
timeout 120 python bench.py --workload roi_align_rotated --no-cpu-baseline --no-secondary 2>/dev/null | tail -1
}

run_g() {
# Round 4: graph-mode divergence bisect (shared-pool / own-pool / eager update), backward A/B (scan folded or not),
# S2ANet with P4 packed with the small levels
R=$PWD
OUT=$R/gpurun_out/r4_g; mkdir -p $OUT
export TMPDIR=/tmp
for m in shared own eager; do
  JDET_GRAPH_UPDATE=$m timeout 600 python scripts/ddp_graph_diag.py orcnn 7 2 > $OUT/ddp_$m.log 2>&1
  echo "== update=$m"; grep -E "RESULT|DISAGREE|GARBAGE" $OUT/ddp_$m.log | cut -c1-330 | head -8
done
trace() {  # $1 = tag, $2 = workload, rest = env
  tag=$1; wl=$2; shift; shift
  (cd /tmp && env "$@" timeout 300 rocprofv3 --kernel-trace --output-format csv -d $OUT/t_$tag -o t -- python $R/bench.py --workload $wl --no-cpu-baseline --no-secondary --steps 50 > $OUT/t_$tag.log 2>&1)
  python - <<PY
import csv,glob,collections,re
f=glob.glob("$OUT/t_$tag/**/*kernel_trace.csv",recursive=True)
d=collections.defaultdict(list)
for r in csv.DictReader(open(f[0])):
    m=re.search(r"((roi|csr|bwd|riroi)_\w+_kernel)", r["Kernel_Name"]); k=m.group(1) if m else r["Kernel_Name"][:30]
    d[k].append((int(r["End_Timestamp"])-int(r["Start_Timestamp"]))/1e3)
tot=sum(sum(v[5:])/len(v[5:]) for k,v in d.items() if len(v)>5)
print("[$tag] total %.1f :"%tot, "; ".join("%s %.1f"%(k,sum(v[5:])/len(v[5:])) for k,v in d.items() if len(v)>5))
PY
}
trace bwd_fold roi_align_rotated_bwd A=1
trace bwd_nofold roi_align_rotated_bwd JDET_ROI_BWD_FOLD_SCAN=0
timeout 300 python -m pytest tests/test_gpu_roi_align.py -x -q -k "channels_last or kept_workspace or cfg0 or full_size" 2>&1 | tail -2
for p in 1024 4096; do JDET_PACK_MAX_POS=$p timeout 600 python bench.py --steps 20 --warmup 5 --no-cpu-baseline --no-secondary 2>/dev/null | tail -1 | python -c 'import sys,json; d=json.loads(sys.stdin.readline()); print("s2anet pack_max_pos='$p'", round(d["value"],2), "img/s", round(d["ms_per_step"],3), "ms")'; done
}

run_h() {
R=$PWD
OUT=$R/gpurun_out/r4_h; mkdir -p $OUT
export TMPDIR=/tmp
timeout 600 python scripts/conv1x1_probe.py 2>&1 | grep -v Warning | tail -20
timeout 900 python -m pytest tests/test_gpu_ddp_detectors.py -q 2>&1 | tail -3
timeout 600 python -m pytest tests/test_gpu_roi_align.py -x -q 2>&1 | tail -2
}

run_i() {
R=$PWD
OUT=$R/gpurun_out/r4_i; mkdir -p $OUT
export TMPDIR=/tmp
timeout 600 python -m pytest tests/test_gpu_conv1x1.py tests/test_gpu_s2anet.py -q 2>&1 | tail -3
for g in 0 1; do JDET_CONV1X1_GEMM=$g timeout 600 python bench.py --steps 20 --warmup 5 --no-cpu-baseline --no-secondary 2>/dev/null | tail -1 | python -c 'import sys,json; d=json.loads(sys.stdin.readline()); print("s2anet conv1x1_gemm='$g'", round(d["value"],2), "img/s", round(d["ms_per_step"],3), "ms")'; done
for g in 0 1; do JDET_CONV1X1_GEMM=$g timeout 600 python bench.py --workload orcnn_train --steps 20 --warmup 5 --no-cpu-baseline --no-secondary 2>/dev/null | tail -1 | python -c 'import sys,json; d=json.loads(sys.stdin.readline()); print("orcnn conv1x1_gemm='$g'", round(d["value"],2), "img/s", round(d["ms_per_step"],3), "ms")'; done
}

run_j() {
R=$PWD
OUT=$R/gpurun_out/r4_j; mkdir -p $OUT
export TMPDIR=/tmp
timeout 2400 python -m pytest tests -q -m gpu -x > $OUT/pytest_gpu.log 2>&1
echo "pytest -m gpu rc=$?"; tail -5 $OUT/pytest_gpu.log
for wl in s2anet_train orcnn_train retinanet_infer roitrans_r50_train; do timeout 600 python bench.py --workload $wl --steps 20 --warmup 5 --no-cpu-baseline --no-secondary 2>/dev/null | tail -1 | python -c 'import sys,json; d=json.loads(sys.stdin.readline()); print("'$wl'", round(d["value"],2), d["unit"], round(d["ms_per_step"],3), "ms")'; done
}

run_k() {
timeout 900 python -m pytest tests/test_gpu_convex_ops.py tests/test_gpu_reference_kernels.py -q -k "convex" 2>&1 | tail -15
}

run_l() {
timeout 900 python -m pytest tests/test_gpu_s2anet.py tests/test_gpu_head_parity.py -q 2>&1 | tail -3
for p in 1024 4096 16384; do JDET_PACK_MAX_POS=$p timeout 600 python bench.py --steps 20 --warmup 5 --no-cpu-baseline --no-secondary 2>/dev/null | tail -1 | python -c 'import sys,json; d=json.loads(sys.stdin.readline()); print("s2anet pack_max_pos='$p'", round(d["value"],2), "img/s", round(d["ms_per_step"],3), "ms")'; done
JDET_PACK_MAX_POS=4096 timeout 600 python bench.py --workload retinanet_infer --steps 30 --warmup 5 --no-cpu-baseline --no-secondary 2>/dev/null | tail -1 | cut -c1-200
}

run_m() {
R=$PWD; OUT=$R/gpurun_out/r4_m; mkdir -p $OUT; export TMPDIR=/tmp
for e in 0 1 0 1; do JDET_BENCH_CHECKSUM=1 JDET_ROI_FWD_EXACT=$e timeout 120 python bench.py --workload roi_align_rotated --no-cpu-baseline --no-secondary 2>$OUT/err_$e.log | tail -1 | python -c 'import sys,json; d=json.loads(sys.stdin.readline()); print("exact='$e'", round(d["ms_per_step"]*1000,2),"us/step", round(d["roofline"]["kernel_ms"]*1000,2), "us (events)")'; grep checksum $OUT/err_$e.log | tail -1; done
(cd /tmp && JDET_ROI_FWD_EXACT=1 timeout 300 rocprofv3 --pmc TCP_TOTAL_CACHE_ACCESSES_sum SQ_INSTS_VMEM_RD --output-format csv -d $OUT/p -o t -- python $R/bench.py --workload roi_align_rotated --no-cpu-baseline --no-secondary --steps 10 --warmup 3 > $OUT/p.log 2>&1)
python - <<PY
import csv,glob,collections
for f in glob.glob("$OUT/p/**/*counter_collection.csv",recursive=True):
    d=collections.defaultdict(lambda: collections.defaultdict(list))
    for r in csv.DictReader(open(f)):
        if "merged" in r["Kernel_Name"]: d["merged"][r["Counter_Name"]].append(float(r["Counter_Value"]))
    print({c: round(sum(x)/len(x)) for c,x in d["merged"].items()})
PY
timeout 600 python -m pytest tests/test_gpu_roi_align.py tests/test_gpu_s2anet.py -x -q 2>&1 | tail -2
}

run_n() {
timeout 900 python scripts/convergence_check.py 2>&1 | grep -v Warning | tail -8
timeout 2400 python -m pytest tests -m gpu -q 2>&1 | tail -2
timeout 600 python bench.py --full 2>/dev/null | tail -1 | cut -c1-700
}

run_o() {
R=$PWD; OUT=$R/gpurun_out/r4_o; mkdir -p $OUT; export TMPDIR=/tmp
for kb in 0 20 26 36 52; do
  (cd /tmp && JDET_ROI_BWD_GATHER_LDS_KB=$kb timeout 300 rocprofv3 --kernel-trace --output-format csv -d $OUT/t_$kb -o t -- python $R/bench.py --workload roi_align_rotated_bwd --no-cpu-baseline --no-secondary --steps 50 > $OUT/t_$kb.log 2>&1)
  python - <<PY
import csv,glob,collections,re
f=glob.glob("$OUT/t_$kb/**/*kernel_trace.csv",recursive=True)
d=collections.defaultdict(list)
for r in csv.DictReader(open(f[0])):
    m=re.search(r"((csr|bwd)_\w+_kernel)", r["Kernel_Name"])
    if m: d[m.group(1)].append((int(r["End_Timestamp"])-int(r["Start_Timestamp"]))/1e3)
print("lds_kb=$kb", "; ".join("%s %.1f"%(k,sum(v[5:])/len(v[5:])) for k,v in d.items() if len(v)>5))
PY
done
for kb in 0 26; do
(cd /tmp && JDET_ROI_BWD_GATHER_LDS_KB=$kb timeout 300 rocprofv3 --pmc TCC_EA0_RDREQ_sum TCC_READ_sum --output-format csv -d $OUT/p_$kb -o t -- python $R/bench.py --workload roi_align_rotated_bwd --no-cpu-baseline --no-secondary --steps 10 --warmup 3 > $OUT/p_$kb.log 2>&1)
python - <<PY
import csv,glob,collections
for f in glob.glob("$OUT/p_$kb/**/*counter_collection.csv",recursive=True):
    d=collections.defaultdict(lambda: collections.defaultdict(list))
    for r in csv.DictReader(open(f)):
        if "gather" in r["Kernel_Name"]: d["gather"][r["Counter_Name"]].append(float(r["Counter_Value"]))
    print("lds_kb=$kb gather", {c: round(sum(x)/len(x)) for c,x in d["gather"].items()})
PY
done
}

run_p() {
R=$PWD; OUT=$R/gpurun_out/r4_p; mkdir -p $OUT
timeout 600 python -m pytest tests/test_gpu_conv_wgrad.py -x -q 2>&1 | tail -3
timeout 600 python scripts/conv_wgrad_timing.py ${KS:-0} 2>&1 | tee $OUT/wgrad_timing.jsonl
}

run_r() {
R=$PWD; OUT=$R/gpurun_out/r4_r; mkdir -p $OUT
timeout 900 python -m pytest tests/test_gpu_conv_wgrad.py tests/test_gpu_dcn_arf.py tests/test_gpu_conv_igemm.py tests/test_gpu_s2anet.py -x -q 2>&1 | tail -8
python scripts/conv_wgrad_timing.py 0 2>&1 | python -c "
import sys, json
for l in sys.stdin:
    if l.startswith('{'):
        d = json.loads(l); print(d['shape'], 'lib', d['lib_us'], 'own', d['own_us_ks0'])"
for cfg in "1 32768" "0 0" "1 0" "1 8192" "1 32768" "0 0"; do
  set -- $cfg
  echo "== JDET_CONV_WGRAD=$1 JDET_DCN_FUSED_TRAIN_MIN_POS=$2"
  JDET_CONV_WGRAD=$1 JDET_DCN_FUSED_TRAIN_MIN_POS=$2 timeout 600 python bench.py --no-cpu-baseline --no-secondary --steps 30 --warmup 8 2>&1 | grep -o '"ms_per_step": [0-9.]*'
done
}

run_s() {
timeout 900 python -m pytest tests/test_gpu_s2anet.py tests/test_gpu_ddp_detectors.py -x -q 2>&1 | tail -4
for v in 1 0 1 0; do
  echo "== JDET_HEAD_STREAMS=$v"
  JDET_HEAD_STREAMS=$v timeout 600 python bench.py --no-cpu-baseline --no-secondary --steps 30 --warmup 8 2>&1 | grep -o '"ms_per_step": [0-9.]*'
done
}

run_t() {
timeout 900 python -m pytest tests/test_gpu_s2anet.py tests/test_gpu_ddp_detectors.py tests/test_gpu_conv1x1.py tests/test_gpu_conv_igemm.py -x -q 2>&1 | tail -4
for v in 1 0 1 0; do
  echo "== JDET_CONV_BWD_STREAMS=$v"
  JDET_CONV_BWD_STREAMS=$v timeout 600 python bench.py --no-cpu-baseline --no-secondary --steps 30 --warmup 8 2>&1 | grep -o '"ms_per_step": [0-9.]*'
done
for v in 1 0; do
  echo "== orcnn JDET_CONV_BWD_STREAMS=$v"
  JDET_CONV_BWD_STREAMS=$v timeout 600 python bench.py --workload orcnn_train --no-cpu-baseline --no-secondary --steps 20 --warmup 6 2>&1 | grep -o '"ms_per_step": [0-9.]*'
done
}

run_v() {
# round 4: the line-dedup forward (csrc/roi_align_line.h, JDET_ROI_FWD_LINE=1): parity suites, then bench + kernel trace A/B
R=$PWD; OUT=$R/gpurun_out/r4_v; mkdir -p $OUT; export TMPDIR=/tmp
JDET_ROI_FWD_LINE=1 timeout 900 python -m pytest tests/test_gpu_roi_align.py tests/test_gpu_reference_kernels.py -q 2>&1 | tail -4
for v in ${LINES:-0 1 0 1}; do
  echo "== JDET_ROI_FWD_LINE=$v"
  JDET_ROI_FWD_LINE=$v timeout 300 python bench.py --workload roi_align_rotated --no-cpu-baseline --no-secondary 2>&1 | grep -o '"ms_per_step": [0-9.]*'
done
for v in ${TRACE:-0 1}; do
  (cd /tmp && JDET_ROI_FWD_LINE=$v timeout 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/t_$v -o t -- python $R/bench.py --workload roi_align_rotated --no-cpu-baseline --no-secondary --steps 50 > $OUT/t_$v.log 2>&1)
  k=$(find $OUT/t_$v -name '*kernel_stats.csv' | head -1); echo "LINE=$v"; head -4 $k | cut -c1-160
  rm -rf $OUT/t_$v
done
if [ "${PMC:-0}" = "1" ]; then
for v in ${TRACE:-0 1}; do
  for c in "TCC_EA0_RDREQ_sum TCC_READ_sum" "TCP_TOTAL_CACHE_ACCESSES_sum TCP_TCC_READ_REQ_sum SQ_INSTS_VMEM_RD SQ_INSTS_VALU SQ_WAVE_CYCLES SQ_WAIT_INST_ANY"; do
    n=$(echo $c | tr ' ' '_' | cut -c1-20)
    (cd /tmp && JDET_ROI_FWD_LINE=$v timeout 300 rocprofv3 --pmc $c --output-format csv -d $OUT/p_${v}_$n -o p -- python $R/bench.py --workload roi_align_rotated --no-cpu-baseline --no-secondary --steps 10 --warmup 3 > $OUT/p_${v}_$n.log 2>&1)
  done
  python - <<PY
import csv, glob, collections
agg = collections.defaultdict(list)
for f in glob.glob("$OUT/p_${v}_*/**/*counter_collection.csv", recursive=True):
    for row in csv.DictReader(open(f)):
        if "roi_align_fwd" in row["Kernel_Name"]: agg[row["Counter_Name"]].append(float(row["Counter_Value"]))
print("LINE=$v", {k: round(sum(x)/len(x)) for k, x in sorted(agg.items())})
PY
  rm -rf $OUT/p_${v}_*/
done
fi
}

run_w() {
# round 4: re-validation after the forward mode 3 commit: smoke, full GPU suite, default bench line
timeout 300 python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -1
timeout 2400 python -m pytest tests -m gpu -q 2>&1 | tail -3
timeout 900 python bench.py --full 2>/dev/null | tail -1 | cut -c1-400
}

run_x() {
# round 4: fused SGD step with the clip folded in (JDET_FUSED_SGD): tests + S2ANet / Oriented R-CNN step A/B
timeout 900 python -m pytest tests/test_gpu_s2anet.py tests/test_gpu_ddp_detectors.py -q 2>&1 | tail -3
for v in 1 0 1 0; do
  echo "== JDET_FUSED_SGD=$v"
  JDET_FUSED_SGD=$v timeout 600 python bench.py --no-cpu-baseline --no-secondary --steps 30 --warmup 8 2>&1 | grep -o '"ms_per_step": [0-9.]*'
done
for v in 1 0; do
  echo "== orcnn JDET_FUSED_SGD=$v"
  JDET_FUSED_SGD=$v timeout 600 python bench.py --workload orcnn_train --no-cpu-baseline --no-secondary --steps 20 --warmup 6 2>&1 | grep -o '"ms_per_step": [0-9.]*'
done
}

run_y() {
# round 4: LevelPack mask fused into the tower convs (JDET_PACK_FUSED_MASK) + RotationInvariantPooling kernels (JDET_RIP_KERNEL)
timeout 900 python -m pytest tests/test_gpu_dcn_arf.py tests/test_gpu_s2anet.py tests/test_gpu_conv_igemm.py tests/test_gpu_head_parity.py -q 2>&1 | tail -3
for cfg in "1 1" "0 0" "1 0" "1 1" "0 0"; do
  set -- $cfg
  echo "== JDET_PACK_FUSED_MASK=$1 JDET_RIP_KERNEL=$2"
  JDET_PACK_FUSED_MASK=$1 JDET_RIP_KERNEL=$2 timeout 600 python bench.py --no-cpu-baseline --no-secondary --steps 30 --warmup 8 2>&1 | grep -o '"ms_per_step": [0-9.]*'
done
}

run_z() {
# round 4: pack / unpack as autograd Functions (JDET_PACK_FUNCTIONS) + channels-last ARF bank (JDET_ARF_CL): step A/B
for cfg in "1 1" "0 0" "1 1" "0 0"; do
  set -- $cfg
  echo "== JDET_PACK_FUNCTIONS=$1 JDET_ARF_CL=$2"
  JDET_PACK_FUNCTIONS=$1 JDET_ARF_CL=$2 timeout 600 python bench.py --no-cpu-baseline --no-secondary --steps 30 --warmup 8 2>&1 | grep -o '"ms_per_step": [0-9.]*'
done
}

run=${1:-}; [ $# -gt 0 ] && shift
case "$run" in
  b|d|e|f|final|fwd|g|h|i|j|k|l|m|n|o|p|r|s|t|v|w|x|y|z) run_$run "$@";;
  *) echo "usage: gpu_r4.sh {b|d|e|f|final|fwd|g|h|i|j|k|l|m|n|o|p|r|s|t|v|w|x|y|z} [args]"; exit 2;;
esac
