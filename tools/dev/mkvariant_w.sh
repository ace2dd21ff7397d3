#!/bin/bash
# development variant of the library with ONLY the (8, 6) table variant of the wave kernel rebuilt (BASELINE config 5):
#   tools/dev/mkvariant_w.sh NAME [-Dmacro ...]  ->  proflib/NAME.so   (the other objects come from the product build)
set -e
cd "$(dirname "$0")/../.."
name=$1; shift
mkdir -p proflib
C=pycllp_amd/csrc
T=$(mktemp -d); trap 'rm -rf "$T"' EXIT
/opt/rocm/bin/hipcc -O3 -std=c++17 --offload-arch=gfx950 -fPIC -Wno-unused-function -DWREG_PART=0 -DPYCLLP_DEV_ONLY_W86 "$@" -c -o $T/ipm_wreg.o $C/ipm_wreg.hip
# the product's object list (the Makefile's), with the object rebuilt above in place of its own
objs=$(for o in $(make -s --no-print-directory -C $C print-objs); do [ -f $T/${o##*/} ] && echo $T/${o##*/} || echo $o; done)
/opt/rocm/bin/hipcc --offload-arch=gfx950 -fPIC -shared -o proflib/$name.so $objs
echo built proflib/$name.so
