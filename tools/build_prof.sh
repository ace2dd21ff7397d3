#!/bin/bash
# diagnostic build with in-kernel phase stamps: proflib/libpycllp_hip_prof.so (use with PYCLLP_HIP_LIB=...)
# The product's Makefile with -DPYCLLP_PROFILE (and $PROF_EXTRA), into a directory of its own: every unit is stamped.
set -e
cd "$(dirname "$0")/.."
mkdir -p proflib
T=$(mktemp -d); trap 'rm -rf "$T"' EXIT
make -s -C pycllp_amd/csrc -j${MAX_JOBS:-10} OUT=$T/ EXTRA="-DPYCLLP_PROFILE $PROF_EXTRA"
cp $T/libpycllp_hip.so proflib/libpycllp_hip_prof.so
ls -la proflib/
