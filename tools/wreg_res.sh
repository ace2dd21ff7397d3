#!/bin/bash
# compile one unit of the wave kernels (UNIT = tab, da, pa, pc, pcda, pcpa, bd or bdpa; default tab) with the product's Makefile and
# print the per-kernel register/scratch summary (no GPU needed)
T=$(mktemp -d); trap 'rm -rf "$T"' EXIT
make -s -C "$(dirname "$0")"/../pycllp_amd/csrc OUT=$T/ EXTRA="$EXTRA -Rpass-analysis=kernel-resource-usage" $T/ipm_wreg_${UNIT:-tab}.o 2>&1 | grep "error\|Function Name\|Scratch\|VGPRs Spill" | sed 's/.*remark: //; s/\[-Rpass.*//; s/_ZN12_GLOBAL__N_1//'
