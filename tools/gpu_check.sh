#!/bin/bash
# GPU-box check run: parity tests, smoke, bench (--full: with the CPU baseline, parity and end-to-end
# parts), kernel-trace profile.  Every GPU step has its own time limit and the script stops at the
# first failure.  Logs and profiles go to OUT_DIR (default: check_out/ in the repository).
set -o pipefail
R="$(cd "$(dirname "$0")/.." && pwd)"
cd "$R" || exit 1
O="${OUT_DIR:-$R/check_out}"
mkdir -p "$O"
export TMPDIR=/tmp
step() { echo "== $1"; }
step pytest
timeout -k 10 600 python -m pytest tests -x -q -m gpu > "$O/pytest_gpu.log" 2>&1 || { tail -40 "$O/pytest_gpu.log"; exit 1; }
tail -3 "$O/pytest_gpu.log"
step smoke
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > "$O/smoke.log" 2>&1 || { tail -30 "$O/smoke.log"; exit 1; }
step bench
timeout -k 10 600 python bench.py --full ${BENCH_ARGS:-} > "$O/bench.log" 2>&1 || { tail -30 "$O/bench.log"; exit 1; }
tail -c 2500 "$O/bench.log"
if [ -n "${PROFILE:-}" ]; then
  step rocprof
  cd /tmp || exit 1
  timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d "$O/prof" -o run -- python3 "$R/bench.py" ${BENCH_ARGS:-} > "$O/prof.log" 2>&1 || { tail -30 "$O/prof.log"; exit 1; }
  find "$O/prof" -name "*kernel_stats.csv" -exec cat {} \;
fi
if [ -n "${PMC:-}" ]; then
  step pmc
  cd /tmp || exit 1
  timeout -k 10 600 rocprofv3 --pmc FETCH_SIZE --output-format csv -d "$O/pmc_fetch" -o pmc -- python3 "$R/bench.py" --steps 1 --warmup 0 > "$O/pmc_fetch.log" 2>&1 || { tail -30 "$O/pmc_fetch.log"; exit 1; }
  timeout -k 10 600 rocprofv3 --pmc WRITE_SIZE --output-format csv -d "$O/pmc_write" -o pmc -- python3 "$R/bench.py" --steps 1 --warmup 0 > "$O/pmc_write.log" 2>&1 || { tail -30 "$O/pmc_write.log"; exit 1; }
  python3 "$R/tools/pmc_summary.py" "$O/pmc_fetch" "$O/pmc_write" k_mpc_wave_group 65536 shared > "$O/pmc_k_solve.json" && cat "$O/pmc_k_solve.json"
fi
if [ -n "${CONFIGS:-}" ]; then
  step configs
  cd "$R" || exit 1
  timeout -k 10 600 python3 tools/bench_configs.py --steps 3 > "$O/configs.log" 2>&1 || { tail -30 "$O/configs.log"; exit 1; }
  cat "$O/configs.log"
fi
