#!/bin/bash
# One GPU-box call at the end of a change: the GPU suite as the driver runs it, smoke(), a short bench line.
cd /tmp && export TMPDIR=/tmp; cd $GRAFT_REPO_ROOT
RESULTS=${RESULTS:-results}                   # where the outputs go
mkdir -p $RESULTS
SECONDS=0
timeout 1500 python -m pytest tests -m gpu -q > $RESULTS/gpu_suite.txt 2>&1
echo "suite ${SECONDS}s"; grep -E "passed|failed" $RESULTS/gpu_suite.txt | tail -2; grep "^FAILED" $RESULTS/gpu_suite.txt | head
python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -1
timeout 400 python bench.py --full --steps 6 --warmup 2 --cpu-seconds 0 --lazy-steps 0 > $RESULTS/bench_round.json 2> $RESULTS/bench_round.err
python tools/bench_line.py $RESULTS/bench_round.json
