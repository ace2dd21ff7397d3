#!/bin/bash
# development variant of the library with ONLY the (8, 6) table variant of the wave kernel rebuilt (BASELINE config 5):
#   tools/dev/mkvariant_w.sh NAME [-Dmacro ...]  ->  proflib/NAME.so   (the other objects come from the product build)
set -e
cd "$(dirname "$0")/../.."
name=$1; shift
mkdir -p proflib
C=pycllp_amd/csrc
T=$(mktemp -d); trap 'rm -rf "$T"' EXIT
# the product's objects (the Makefile's list) next to the one rebuilt here: make finds them up to date and links
make -s -C $C OUT=$T/ EXTRA="-DPYCLLP_DEV_ONLY_W86 $*" $T/ipm_wreg_tab.o
for o in $(make -s --no-print-directory -C $C print-objs); do [ -f $T/${o##*/} ] || cp -p $o $T/; done
make -s -C $C OUT=$T/
cp $T/libpycllp_hip.so proflib/$name.so
echo built proflib/$name.so
