#!/bin/bash
# development variant of the library for same-box A/B runs: tools/dev/mkvariant.sh NAME [-Dmacro ...]
# builds ONLY the (32, 96) group kernels of ipm_dense.hip (PYCLLP_DEV_ONLY_3296) with the given macros and links them with the
# product's other objects into proflib/NAME.so (use with PYCLLP_HIP_LIB=$GRAFT_REPO_ROOT/proflib/NAME.so)
set -e
cd "$(dirname "$0")/../.."
name=$1; shift
mkdir -p proflib
C=pycllp_amd/csrc
T=$(mktemp -d); trap 'rm -rf "$T"' EXIT
/opt/rocm/bin/hipcc -O3 -std=c++17 --offload-arch=gfx950 -fPIC -Wno-unused-function -DPYCLLP_DEV_ONLY_3296 "$@" -c -o $T/ipm_dense.o $C/ipm_dense.hip
# the product's object list (the Makefile's), with the object rebuilt above in place of its own
objs=$(for o in $(make -s --no-print-directory -C $C print-objs); do [ -f $T/${o##*/} ] && echo $T/${o##*/} || echo $o; done)
/opt/rocm/bin/hipcc --offload-arch=gfx950 -fPIC -shared -o proflib/$name.so $objs
echo built proflib/$name.so
