# Measurement pass of the round on an MI355X: kernel trace, PMC traffic of the MLP kernels, the full bench line.   usage: [PROFILE_OUT=dir] call_profile.sh [tag]
R=${GRAFT_REPO_ROOT:-/root/repo}
T=${1:-r03}
O=${PROFILE_OUT:-/tmp/avc_profile}
cd /tmp && export TMPDIR=/tmp
rm -rf /tmp/pmcs /tmp/kt && mkdir -p /tmp/pmcs $O
rocprofv3 --kernel-trace --stats -d /tmp/kt -o kt -- python $R/bench.py --steps 6 --warmup 5 --no-cpu-baseline --no-extra > /tmp/kt.log 2>&1
python $R/scripts/rocpd_stats.py /tmp/kt 30 > $O/${T}_bench_512_kernel_trace_stats.txt 2>&1
python $R/scripts/rocpd_gaps.py /tmp/kt 5 | tail -15 >> $O/${T}_bench_512_kernel_trace_stats.txt 2>&1
python $R/scripts/rocpd_census.py /tmp/kt > $O/${T}_step_census.txt 2>&1
for c in FETCH_SIZE WRITE_SIZE; do
  rocprofv3 --pmc $c --kernel-trace --output-format csv -d /tmp/pmcs/$c -o p -- python $R/bench.py --steps 1 --warmup 3 --no-cpu-baseline --no-extra > /tmp/pmc_$c.log 2>&1
done
python $R/scripts/pmc_summary.py /tmp/pmcs --json $O/${T}_pmc_traffic.json "$(cat $O/.commit 2>/dev/null || cat $R/.commit_id 2>/dev/null || echo unknown)" "MI355X box" 4 512 64 > $O/${T}_pmc_fetch_write.txt 2>&1
cp $O/${T}_pmc_traffic.json $R/profiles/ 2>/dev/null   # for the bench run below on THIS box; afterwards commit $O/${T}_* under profiles/
cd $R && python bench.py --full > $O/${T}_bench_512.json 2> $O/${T}_bench_512.err
tail -c 4000 $O/${T}_bench_512.json; echo; head -12 $O/${T}_bench_512_kernel_trace_stats.txt; tail -6 $O/${T}_pmc_fetch_write.txt
