# kernel trace of bench.py's pm_scan leg (--full --scan-passes 3), -K 2.  Usage (GPU box): bash scripts/kt_scan.sh <output dir>
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
out=${1:?output directory}/kt_scan
mkdir -p $out
rocprofv3 --kernel-trace --stats --output-format csv -d $out/K2 -- python3 bench.py --full --steps 1 --warmup 1 --no-cpu --scan-passes 3 > $out/K2.log 2>&1
echo rc=$?
f=$(ls $out/K2/*/*kernel_stats.csv | tail -1)
cut -d, -f1-4 $f | cut -c1-160 | head -30
