# One GPU iteration: the whole GPU suite, the default bench line with its roofline (no CPU leg) and the in-graph
# bs16 layer profile.  usage: bash scripts/gpu_iter.sh TAG [pytest -k expr]   (results in $YDBL_OUT/TAG, default out/TAG)
cd "$(dirname "$0")/.."; O=${YDBL_OUT:-out}/${1:-it}; mkdir -p $O
K=${2:+-k "$2"}
eval timeout -k 10 900 python -u -m pytest tests -m gpu -x -q --timeout 200 --timeout-method thread -p no:cacheprovider $K \
  > $O/pytest_gpu.log 2>&1; rc=$?; tail -2 $O/pytest_gpu.log; [ $rc -eq 0 ] || exit $rc
timeout -k 10 300 python bench.py --full --no-cpu-baseline > $O/bench.json 2>$O/bench.err || exit 1
cut -c1-400 $O/bench.json
timeout -k 10 200 python scripts/layer_profile.py --batch 16 > $O/layers_bs16.txt 2>&1 || exit 1
head -16 $O/layers_bs16.txt
