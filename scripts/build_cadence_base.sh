#!/bin/bash
# The baseline library of scripts/bench_cadence.py (BASELINE.md "GST-cadence clocks"): this tree
# with the kernel and view sources of commit REV (the parent of the GST-cadence change) overlaid,
# so only the generator change (gst_ppm) is kept -- the parent's read path on the new workload.
# REV's am_pack.hip gets scripts/cadence_base_view_stats.inc appended (a counters-only
# am_store_view_stats; REV has none).  Installs scripts/ab/lib_base.so (scripts/build_variant.sh).
#   scripts/build_cadence_base.sh <REV>;  AM_LIB=scripts/ab/lib_base.so python scripts/bench_cadence.py ...
set -eu
cd "$(dirname "$0")/.."
REV=${1:?usage: build_cadence_base.sh <parent rev>}
T=$(mktemp -d)
trap 'rm -rf "$T"' EXIT
git show "$REV:antidote_amd/csrc/am_pack.hip" > "$T/am_pack.hip"
cat scripts/cadence_base_view_stats.inc >> "$T/am_pack.hip"
H=git:$REV:antidote_amd/csrc
bash scripts/build_variant.sh base "$T/am_pack.hip=am_pack.hip" $H/am_apply.hip=am_apply.hip $H/am_wave.h=am_wave.h \
  $H/am_group.h=am_group.h $H/am_lanes.hip=am_lanes.hip $H/am_bcrows.hip=am_bcrows.hip $H/am_bcwave.hip=am_bcwave.hip \
  $H/am_big.hip=am_big.hip $H/am_rows.hip=am_rows.hip $H/am_runtime.hip=am_runtime.hip $H/am_internal.h=am_internal.h
