#!/bin/bash
# list the scratch (spill) instructions inside the iteration loop of one wave kernel (default: ipm, MB=8, NQ=6) of one unit
# (UNIT = tab, da, pa, pc, pcda, pcpa or bd; default tab).  The product's Makefile with -S: the "object" it writes is the
# device assembly.
K=${1:-ipm_wreg_kernelILi8ELi6E}
mkdir -p /tmp/asm
make -s -B -C "$(dirname "$0")"/../pycllp_amd/csrc OUT=/tmp/asm/ EXTRA="$EXTRA -S --cuda-device-only" /tmp/asm/ipm_wreg_${UNIT:-tab}.o 2>/dev/null
cd /tmp/asm && mv ipm_wreg_${UNIT:-tab}.o wreg.s
a=$(grep -n "^_ZN.*${K}.*:" wreg.s | head -1 | cut -d: -f1)
b=$(awk -v a=$a 'NR>a && /^\.Lfunc_end/{print NR; exit}' wreg.s)
sed -n "${a},${b}p" wreg.s > k.s
h=$(grep -n "This Loop Header: Depth=2" k.s | head -1 | cut -d: -f1)
echo "iteration loop starts at line $h of /tmp/asm/k.s; scratch ops inside:"
grep -n "scratch_" k.s | awk -F: -v h=$h '$1>h' | cut -c1-95
