#!/bin/bash
# diagnostic build with in-kernel phase stamps: proflib/libpycllp_hip_prof.so (use with PYCLLP_HIP_LIB=...)
# (the per-problem-A, predictor-corrector and bounded wave kernels are linked unstamped from the product build)
set -e
cd "$(dirname "$0")/.."
mkdir -p proflib
F="-O3 -std=c++17 --offload-arch=gfx950 -fPIC -Wno-unused-function -DPYCLLP_PROFILE"
C=pycllp_amd/csrc
T=$(mktemp -d); trap 'rm -rf "$T"' EXIT
/opt/rocm/bin/hipcc $F -DWREG_PART=0 -c -o $T/ipm_wreg.o $C/ipm_wreg.hip &
/opt/rocm/bin/hipcc $F -DWREG_PART=1 -c -o $T/ipm_wreg_da.o $C/ipm_wreg.hip &
/opt/rocm/bin/hipcc $F $PROF_EXTRA -c -o $T/ipm_dense.o $C/ipm_dense.hip &
/opt/rocm/bin/hipcc $F -c -o $T/ipm_big.o $C/ipm_big.hip &
wait
# the product's object list (the Makefile's), with the objects rebuilt above in place of theirs
objs=$(for o in $(make -s --no-print-directory -C $C print-objs); do [ -f $T/${o##*/} ] && echo $T/${o##*/} || echo $o; done)
/opt/rocm/bin/hipcc --offload-arch=gfx950 -fPIC -shared -o proflib/libpycllp_hip_prof.so $objs
ls -la proflib/
