#!/bin/bash
# The bench's headline regime under rocprofv3, per stream count (default "4 1"):
#   1. --kernel-trace            -> start/end of every prep, raster and finalize;
#                                   tools/stream_trace.py turns them into queue delays,
#                                   durations and raster overlap over the timed pass
#   2. --pmc SQ_* (its own run)  -> the raster's VALU busy per dispatch.  rocprofv3
#                                   collects counters with the dispatches serialised,
#                                   so this is each raster alone, whatever --streams says
# Outputs under $GGS_OUT_DIR (default out/) streams_<tag>/s<streams>/.
#   LIB=libggs_parent tools/profile_streams.sh parent      (another build: GGS_LIB)
set -u
cd "$(dirname "$0")/.."
ROOT=${GGS_OUT_DIR:-out}
TAG=${1:-new}
STREAMS=${STREAMS:-"4 1"}
STEPS=${STEPS:-200}
L=${LIB:-libggs}
export GGS_LIB=$PWD/genetic-gaussian-splats_amd/$L.so TMPDIR=/tmp
for S in $STREAMS; do
  OUT=$ROOT/streams_$TAG/s$S
  mkdir -p "$OUT"
  BENCH="python3 bench.py --streams $S --steps $STEPS --warmup 20 --ramp-ms 100 --full --extras 0 --no-cpu-baseline"
  echo "$L: $BENCH" > "$OUT/commands.txt"
  timeout -k 10 240 rocprofv3 --kernel-trace -d "$OUT/trace" -o run --output-format csv -- $BENCH \
      > "$OUT/trace.log" 2>&1 || { echo "trace s$S failed"; tail -20 "$OUT/trace.log"; exit 1; }
  python3 tools/stream_trace.py "$OUT/trace" --steps "$STEPS" > "$OUT/stream_trace.json" || exit 1
  cat "$OUT/stream_trace.json"
  timeout -k 10 240 rocprofv3 --pmc SQ_WAVES SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_WAVE_CYCLES GRBM_GUI_ACTIVE \
      --kernel-include-regex raster_kernel -d "$OUT/pmc_sq" -o run --output-format csv -- $BENCH \
      > "$OUT/pmc.log" 2>&1 || { echo "pmc s$S failed"; tail -20 "$OUT/pmc.log"; exit 1; }
  python3 tools/stream_pmc.py "$OUT/pmc_sq" > "$OUT/pmc_summary.json" || exit 1
  cat "$OUT/pmc_summary.json"
done
