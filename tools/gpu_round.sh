#!/bin/bash
# One GPU-box session: op parity, model parity, bench, (optional) rocprof.  Everything lands in $OUT (default: logs/).
# usage: [OUT=dir] tools/gpu_round.sh [stages...]   stages: ops models bench benchq prof smoke
set -u
cd "$(dirname "$0")/.."
ROOT=$PWD
mkdir -p "${OUT:=logs}" && OUT=$(cd "$OUT" && pwd)
export TMPDIR=/tmp
STAGES="${@:-ops models bench}"
python -c "import torch;print('torch',torch.__version__,'gpu',torch.cuda.get_device_name(0))" 2>&1 | tee "$OUT/env.log"
nproc | tee -a "$OUT/env.log"
for s in $STAGES; do
  case $s in
    ops)    timeout 900 python -m pytest tests/test_ops_gpu.py -m gpu -q -rA --timeout=300 -p no:cacheprovider > "$OUT/pytest_ops.log" 2>&1; echo "ops rc=$?";;
    models) timeout 1500 python -m pytest tests/test_models_gpu.py -m gpu -q -rA --timeout=900 -p no:cacheprovider > "$OUT/pytest_models.log" 2>&1; echo "models rc=$?";;
    bench)  timeout 900 python bench.py --full --steps 2 --warmup 1 > "$OUT/bench.log" 2> "$OUT/bench.err"; echo "bench rc=$?"; tail -c 3000 "$OUT/bench.log";;
    benchq) timeout 600 python bench.py --full --steps 2 --warmup 1 --no-cpu-baseline > "$OUT/bench.log" 2> "$OUT/bench.err"; echo "bench rc=$?"; tail -c 3000 "$OUT/bench.log";;
    prof)   (cd "$TMPDIR" && timeout 900 rocprofv3 --kernel-trace --stats -d "$OUT/prof" -o r1 -- python "$ROOT/bench.py" --steps 1 --warmup 1 --no-cpu-baseline --no-roofline > "$OUT/prof.log" 2>&1); echo "prof rc=$?";;
    smoke)  timeout 600 python -c "import __graft_entry__ as g; g.smoke()" > "$OUT/smoke.log" 2>&1; echo "smoke rc=$?"; tail -3 "$OUT/smoke.log";;
  esac
done
for f in "$OUT/pytest_ops.log" "$OUT/pytest_models.log"; do [ -f "$f" ] && { echo "== $f"; grep -E "^(PASSED|FAILED|ERROR)|passed|failed" "$f" | tail -80; }; done
[ -s "$OUT/bench.err" ] && { echo "== bench.err"; tail -30 "$OUT/bench.err"; }
exit 0
