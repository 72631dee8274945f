# The r08 set: conv_ws64_kernel reading each fragment set once, against a build of the parent commit, both libraries alternating in ONE call
# on one box.  run_r08_ws64.sh <parent's libmfpa.so> [<this commit's> [<output directory, default build/r08>]]   (copy the files to profiles/r08_*)
#   ws64_speed_pairs.txt   tools/ab_ws64_libs.sh: the six routed launches at 128 clips, three rounds of three readings of 40 launches
#   bench_line_parent_{1,2,3}.json, bench_line_{1,2,3}.json   bench.py --lib <...> --steps 20 --warmup 5, three pairs
#   pmc_sq_pass{1,2}[_parent].json, pmc_sq_table.md   two SQ counter passes (--pmc alone, no tracing) of ONE 64-clip forward per library
# Every GPU step runs under its own time limit and the script stops at the first step that fails.
set -o pipefail
export TMPDIR=/tmp
P=${1:?parent library}; N=${2:-musicfpaugment_amd/libmfpa.so}
O=${3:-build/r08}; mkdir -p $O
ROUNDS=3 REPS=40 READINGS=3 bash tools/ab_ws64_libs.sh 128 $P $N > $O/ws64_speed_pairs.txt 2>&1 || { tail -5 $O/ws64_speed_pairs.txt; exit 1; }
for i in 1 2 3; do
  timeout -k 10 240 python bench.py --lib $P --steps 20 --warmup 5 > $O/bench_line_parent_$i.json 2> $O/bench_parent_$i.err || exit 1
  timeout -k 10 240 python bench.py --lib $N --steps 20 --warmup 5 > $O/bench_line_$i.json 2> $O/bench_$i.err || exit 1
done
FAM=conv_mfma_kernel,convT_mfma_kernel,conv_wd16_kernel,conv_ws64_kernel,conv_up_kernel
S1="SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_VALU_MFMA_BUSY_CYCLES SQ_WAIT_INST_LDS GRBM_GUI_ACTIVE"
S2="SQ_INSTS_VALU SQ_INSTS_MFMA SQ_INSTS_LDS SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS SQ_INSTS_SALU"
for who in _parent ""; do
  L=$N; [ -n "$who" ] && L=$P
  CMD="python3 bench.py --lib $L --clips 64 --steps 1 --warmup 0 --cpu-seconds 0 --no-configs --no-extras"
  timeout -k 10 400 rocprofv3 --pmc $S1 -d $O/pmc_s1 -o p --output-format csv -- $CMD > $O/pmc_s1$who.log 2>&1 || exit 1
  timeout -k 10 400 rocprofv3 --pmc $S2 -d $O/pmc_s2 -o p --output-format csv -- $CMD > $O/pmc_s2$who.log 2>&1 || exit 1
  python tools/summarize_sq.py $O/pmc_s1 $FAM $O/pmc_sq_pass1$who.json > /dev/null || exit 1
  python tools/summarize_sq.py $O/pmc_s2 $FAM $O/pmc_sq_pass2$who.json > /dev/null || exit 1
  rm -rf $O/pmc_s1 $O/pmc_s2
done
{ echo "One 64-clip bf16x3 forward per library, two \`rocprofv3 --pmc\` passes each (no tracing), both libraries in one call on one box."; echo
  echo "Parent commit:"; echo; python tools/sq_table.py $O/pmc_sq_pass1_parent.json $O/pmc_sq_pass2_parent.json; echo
  echo "This commit (\`conv_ws64_kernel\` reads each fragment set once and takes its weight fragments through raw buffer loads; the other kernels are unchanged):"; echo
  python tools/sq_table.py $O/pmc_sq_pass1.json $O/pmc_sq_pass2.json; } > $O/pmc_sq_table.md
python - <<PY
import json
v = {n: [json.loads(open("$O/bench_line%s_%d.json" % (n, i)).read().strip().splitlines()[-1]) for i in (1, 2, 3)] for n in ("_parent", "")}
for i in range(3):
    a, b = v["_parent"][i], v[""][i]
    print("pair %d: %.1f (%.3f ms) | %.1f (%.3f ms)  %+.2f %%" % (i + 1, a["value"], a["ms_per_step"], b["value"], b["ms_per_step"], 100 * (b["value"] / a["value"] - 1)))
PY
grep ws64 $O/pmc_sq_table.md
