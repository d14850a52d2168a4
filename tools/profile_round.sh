# Round profile: bench line (--full), rocprofv3 kernel trace of the same command, and the two HBM counter passes (one counter per pass, the decision kernel only) on the very
# launch shape that is timed: 600 frames (the ten-wave build, frames migrating between workgroups).
# usage (on a machine with an MI355X): bash tools/profile_round.sh <tag> [output directory, default profile_out]
set -x
TAG=${1:-r04}
export TMPDIR=/tmp
R=$(cd "$(dirname "$0")/.." && pwd)
cd $R
D=${2:-profile_out}
mkdir -p $D
python bench.py --full --steps 3 --warmup 1 > $D/${TAG}_bench.json 2> $D/${TAG}_bench.err
Q="--steps 1 --warmup 0"
rocprofv3 --kernel-trace --stats -d $D/${TAG}_trace -o ${TAG} -- python bench.py $Q > $D/${TAG}_trace.log 2>&1
QC="--frames 600 $Q"
timeout 900 rocprofv3 --pmc FETCH_SIZE --kernel-include-regex hevcdl_rd_frame_kernel -d $D/${TAG}_fetch -o ${TAG} -- python bench.py $QC > $D/${TAG}_fetch.log 2>&1
timeout 900 rocprofv3 --pmc WRITE_SIZE --kernel-include-regex hevcdl_rd_frame_kernel -d $D/${TAG}_write -o ${TAG} -- python bench.py $QC > $D/${TAG}_write.log 2>&1
python tools/rocpd_summary.py $D/${TAG}_trace $D/${TAG}_fetch $D/${TAG}_write > $D/${TAG}_summary.txt 2>&1
sha256sum hevc-deep-learning-pipeline_amd/csrc/rd_kernel.hip | cut -c1-16 > $D/${TAG}_rd_kernel_sha16.txt
tail -1 $D/${TAG}_bench.json | cut -c1-300
grep -E 'hevcdl|##' $D/${TAG}_summary.txt | cut -c1-160
# the rocpd databases are tens of MB each: keep the summaries, drop the databases
rm -rf $D/${TAG}_trace $D/${TAG}_fetch $D/${TAG}_write
