#!/bin/bash
# build wfbench variants HERE (cross-compiled): run_wfbench.sh build <name> [kernel-header-dir] [-D flags...]
#   `base` is usually built once from a saved copy of thaler-study_amd/csrc (tools/build/base_csrc, made by `save-base`)
# on the GPU box: run_wfbench.sh run <logs...>   alternates every built variant three times; the first run that fails or
#   outlives its time limit ends the script.  WF_SLOTS / WF_ALT / WF_SHAPE / WF_REPS (wfbench.hip) are passed on: the settings of
#   the clock-aligned write slots are run-time knobs of ONE build, e.g.
#     WF_SLOTS=0:0:0,800:0:0,800:0:1,800:600:0,800:600:1 run_wfbench.sh run 28
#   (a build from headers without the slots runs the 0:0:0 entries only)
#   run_wfbench.sh clocks   builds nothing: runs tools/build/xcd_clock_probe (build it with `build-clocks`), the precondition of the slots
set -e
cd "$(dirname "$0")"
mkdir -p build
case "$1" in
  save-base) rm -rf build/base_csrc; cp -r ../thaler-study_amd/csrc build/base_csrc; rm -rf build/base_csrc/build; echo saved;;
  build) name=$2; dir=${3:-../thaler-study_amd/csrc}; shift; shift; shift || true
         /opt/rocm/bin/hipcc -O3 -std=c++17 --offload-arch=gfx950 -DKERNELS_HPP="\"$(realpath $dir)/kernels.hpp\"" "$@" -o build/wfbench_$name wfbench.hip
         ls -la build/wfbench_$name;;
  build-clocks) /opt/rocm/bin/hipcc -O3 -std=c++17 --offload-arch=gfx950 -o build/xcd_clock_probe xcd_clock_probe.hip
         ls -la build/xcd_clock_probe;;
  clocks) timeout -k 10 120 build/xcd_clock_probe;;
  run) shift
       for rep in 1 2 3; do for b in build/wfbench_*; do timeout -k 10 600 $b $(basename $b | sed s/wfbench_//) "$@"; done; done;;
esac
