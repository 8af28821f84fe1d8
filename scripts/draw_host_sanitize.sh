#!/bin/bash
# The device episode generators' host-only pieces -- the table of draw kinds (mv_draw.h), mv_debug_draw_host and the host twins (mv_draw.hip, mv_*_draw.hip),
# with the host generators and the scenario table they are linked against -- built with AddressSanitizer and UBSan into a stand-alone program and run.
# No GPU involved; nothing that Python loads is built this way.  usage: scripts/draw_host_sanitize.sh
set -e
R=$(cd "$(dirname "$0")/.." && pwd); C=$R/megaverse_amd/csrc; T=$(mktemp -d)
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -fno-fast-math -Wno-unused-function -Wno-pass-failed \
  -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined -Xarch_host -fno-omit-frame-pointer \
  -o $T/draw_host_sanitize $R/scripts/draw_host_sanitize.cpp $C/mv_draw.hip $C/mv_collect_draw.hip $C/mv_obstacles_draw.hip $C/mv_hex_draw.hip \
  $C/mv_scenarios.cpp $C/mv_gen_*.cpp
ASAN_OPTIONS=detect_leaks=0 $T/draw_host_sanitize; rc=$?   # (leaks: the HIP runtime's start-up allocations are not this program's)
rm -rf $T; exit $rc
